// The part of row_units.hpp that is plain C++ as well: the band rule, a lane's walk over a band with the lane as an argument, and byte_perm
// with a host equivalent, so that lane bodies written against a thread index run on the CPU too (image_unpack_body.hpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VSZIP_HD __host__ __device__ __forceinline__
#else
#define VSZIP_HD inline
#endif

constexpr int kRowUnitThreads = 256;

// Rows a workgroup takes of a frame whose rows are `units` lane-units long: as many as fill the workgroup once, one from 256 units on, 16 at the
// most. Measured with both kernels at 1, 2, 4 and 8 rows: the fastest band was each time the one nearest to one sweep of the
// workgroup (1080p rows of 120 units: 2 rows; 4K rows of 240 and all rows of 480 or more: 1), longer bands lost 4 to 30 %.
inline int vszip_rows_per_workgroup(int units) { return units >= kRowUnitThreads ? 1 : units <= kRowUnitThreads / 16 ? 16 : kRowUnitThreads / units; }

// f(row, i) for every unit i in [0, n) of every row in [0, rows), the units taken in raster order over the whole band: lane tid starts at
// unit tid and steps by the workgroup's size, so a row shorter than the workgroup leaves no lane idle (a 1080p row of 8-bit samples is
// 120 units of 16 samples). One division a lane; the step is the same (quotient, remainder) for every lane.
template <typename F>
VSZIP_HD void for_each_row_unit(int tid, int rows, int n, F f) {
    if (n <= 0) return;
    const int q = kRowUnitThreads / n, rem = kRowUnitThreads - q * n;
    int row = tid / n, i = tid - row * n;
    while (row < rows) {
        f(row, i);
        row += q;
        i += rem;
        if (i >= n) {
            i -= n;
            ++row;
        }
    }
}

// the 32-bit word whose byte k is byte sel[k] of the eight bytes {hi, lo} (0..3: lo, 4..7: hi; 0x0c: 0x00; 0x0d: 0xFF): v_perm_b32
VSZIP_HD uint32_t byte_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t both = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; ++k) {
        const uint32_t s = (sel >> (8 * k)) & 255u;
        const uint32_t b = s < 8 ? (uint32_t)(both >> (8 * s)) & 255u : s == 0x0d ? 255u : 0u;  // (selectors the kernels do not use read as 0x0c)
        r |= b << (8 * k);
    }
    return r;
#endif
}
