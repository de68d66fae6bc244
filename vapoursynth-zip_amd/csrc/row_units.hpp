// A workgroup's lanes over a band of rows, for the streaming kernels whose planes differ in number or sample width (pack_rgb.hip,
// color_map.hip) and so do not fit stream_map_rows of plane_table.hpp.
#pragma once
#include "plane_table.hpp"

constexpr int kRowUnitThreads = 256;

// Rows a workgroup takes of a frame whose rows are `units` lane-units long: as many as fill the workgroup once, one from 256 units on, 16 at the
// most. Measured with both kernels at 1, 2, 4 and 8 rows: the fastest band was each time the one nearest to one sweep of the
// workgroup (1080p rows of 120 units: 2 rows; 4K rows of 240 and all rows of 480 or more: 1), longer bands lost 4 to 30 %.
inline int vszip_rows_per_workgroup(int units) { return units >= kRowUnitThreads ? 1 : units <= kRowUnitThreads / 16 ? 16 : kRowUnitThreads / units; }

#if defined(__HIPCC__)
// f(row, i) for every unit i in [0, n) of every row in [0, rows), the units taken in raster order over the whole band: lane t starts at
// unit t and steps by the workgroup's size, so a row shorter than the workgroup leaves no lane idle (a 1080p row of 8-bit samples is
// 120 units of 16 samples). One division a lane; the step is the same (quotient, remainder) for every lane.
template <typename F>
__device__ __forceinline__ void for_each_row_unit(int rows, int n, F f) {
    if (n <= 0) return;
    const int q = kRowUnitThreads / n, rem = kRowUnitThreads - q * n;
    int row = (int)threadIdx.x / n, i = (int)threadIdx.x - row * n;
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
__device__ __forceinline__ uint32_t byte_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
#endif  // __HIPCC__
