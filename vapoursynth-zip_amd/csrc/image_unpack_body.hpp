// The per-lane bodies of the ImageUnpack kernels (image_unpack.hip), written against a thread index given as an argument, so that the
// same text runs as host code too: a stand-alone program calls them for tid = 0 .. 255 of every workgroup over heap blocks of the exact
// size, under AddressSanitizer / UBSan (tests/image_unpack_body_check.cpp); where the kernel has a barrier, the program runs every lane
// up to it before any lane goes on. Only the memory helpers and align_byte here, and byte_perm of row_walk.hpp, differ between the two
// compilations; the walk over a band (for_each_row_unit with the lane as an argument) is row_walk.hpp's, too.
//
// A pixel is C samples of S bytes, interleaved. A lane takes a unit of G = 16 / S pixels: 16 C bytes from any byte address, separated in
// registers into 16 bytes a channel. unit_byte() is the whole layout: which source byte lands in which byte of which output dword.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>

#include "row_walk.hpp"

namespace image_unpack {

constexpr int kThreads = kRowUnitThreads;

struct UnpackFrame {
    const uint8_t *src;
    void *o[4];        // the plane of channel c in the pixel's memory order; nullptr: the channel is dropped (alpha only)
    int ss;            // source pitch in BYTES
    int os[4];         // output pitches in samples
    int w, h;
    short vec, rows;   // every output base and pitch is a multiple of 16 bytes; rows a workgroup
    int block0;
};

// ---- what differs between device and host ----------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_unaligned __attribute__((aligned(1)));

// 16 bytes from any byte address, read once
VSZIP_HD void load16(uint32_t *d, const uint8_t *p) {
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_unaligned *>(p));
    d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
}
// 16 bytes from a global address that is a multiple of 16 to an LDS address that is one
VSZIP_HD void stage16(uint32_t *lds, const uint8_t *p) { *reinterpret_cast<u32x4 *>(lds) = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p)); }
// the dword that starts `sh` bytes into {hi, lo}: v_alignbyte_b32
VSZIP_HD uint32_t align_byte(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
// 16 bytes to an address that is a multiple of 16 (the unit path), written once
VSZIP_HD void store16(uint8_t *p, const uint32_t *d) {
    u32x4 v;
    v.x = d[0], v.y = d[1], v.z = d[2], v.w = d[3];
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(p));
}
#else
inline void stage16(uint32_t *lds, const uint8_t *p) { std::memcpy(lds, p, 16); }
inline uint32_t align_byte(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (sh & 3u))); }
inline void load16(uint32_t *d, const uint8_t *p) { std::memcpy(d, p, 16); }
inline void store16(uint8_t *p, const uint32_t *d) { std::memcpy(p, d, 16); }
#endif

// one sample of S bytes at any byte address, as bits
template <int S>
VSZIP_HD uint32_t load_sample(const uint8_t *p) {
    if constexpr (S == 1) return *p;
    uint32_t v = 0;
    if constexpr (S == 2) v = (uint32_t)p[0] | ((uint32_t)p[1] << 8);
    if constexpr (S == 4) __builtin_memcpy(&v, p, 4);
    return v;
}
// outputs are planes of their sample type: aligned to S
template <int S>
VSZIP_HD void store_sample(uint8_t *p, uint32_t v) {
    if constexpr (S == 1) *p = (uint8_t)v;
    if constexpr (S == 2) *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    if constexpr (S == 4) *reinterpret_cast<uint32_t *>(p) = v;
}

// ---- the layout -------------------------------------------------------------------------------------------------------------------
// the unit's source byte that becomes byte i of dword k of channel c: a dword holds 4 / S samples, sample j of it is pixel k * 4 / S + j
constexpr int unit_byte(int S, int C, int c, int k, int i) { return ((k * (4 / S) + i / S) * C + c) * S + i % S; }

// the dword whose bytes are bytes O0 .. O3 of in[]: nothing (they are one dword), one v_perm_b32 (they lie in two dwords) or three
template <int O0, int O1, int O2, int O3>
VSZIP_HD uint32_t pick(const uint32_t *in) {
    constexpr int a = O0 / 4, b = O1 / 4 != a ? O1 / 4 : O2 / 4 != a ? O2 / 4 : O3 / 4 != a ? O3 / 4 : a;
    constexpr auto in_ab = [](int o) { return o / 4 == a || o / 4 == b; };
    if constexpr (in_ab(O1) && in_ab(O2) && in_ab(O3)) {
        constexpr auto sel = [](int o) { return (uint32_t)((o / 4 == a ? 0 : 4) + o % 4); };
        constexpr uint32_t s = sel(O0) | (sel(O1) << 8) | (sel(O2) << 16) | (sel(O3) << 24);
        if constexpr (s == 0x03020100u) return in[a];
        return byte_perm(in[b], in[a], s);
    } else {
        const uint32_t lo = byte_perm(in[O1 / 4], in[O0 / 4], (uint32_t)(O0 % 4) | ((uint32_t)(4 + O1 % 4) << 8) | 0x0c0c0000u);
        const uint32_t hi = byte_perm(in[O3 / 4], in[O2 / 4], (uint32_t)(O2 % 4) | ((uint32_t)(4 + O3 % 4) << 8) | 0x0c0c0000u);
        return byte_perm(hi, lo, 0x05040100u);
    }
}
template <int S, int C, int c, int k>
VSZIP_HD uint32_t channel_dword(const uint32_t *in) {
    return pick<unit_byte(S, C, c, k, 0), unit_byte(S, C, c, k, 1), unit_byte(S, C, c, k, 2), unit_byte(S, C, c, k, 3)>(in);
}
template <int S, int C, int c, int... K>
VSZIP_HD void channel(const uint32_t *in, uint32_t *o, std::integer_sequence<int, K...>) {
    ((o[K] = channel_dword<S, C, c, K>(in)), ...);
}
// four pixels of four bytes, a dword each -> a dword a channel: the 4 x 4 byte transpose in eight v_perm_b32 (pick<> would take twelve)
VSZIP_HD void transpose4(const uint32_t *d, uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3) {
    const uint32_t t0 = byte_perm(d[1], d[0], 0x05010400u), t1 = byte_perm(d[1], d[0], 0x07030602u);  // c0 c0 c1 c1; c2 c2 c3 c3 of pixels 0, 1
    const uint32_t u0 = byte_perm(d[3], d[2], 0x05010400u), u1 = byte_perm(d[3], d[2], 0x07030602u);  // of pixels 2, 3
    c0 = byte_perm(u0, t0, 0x05040100u);
    c1 = byte_perm(u0, t0, 0x07060302u);
    c2 = byte_perm(u1, t1, 0x05040100u);
    c3 = byte_perm(u1, t1, 0x07060302u);
}
// in[]: the G * C * S bytes of a unit -> out[c][]: the G * S bytes of channel c
template <int S, int C, int G>
VSZIP_HD void separate(const uint32_t *in, uint32_t (&out)[C][G * S / 4]) {
    constexpr int ND = G * S / 4;
    if constexpr (S == 1 && C == 4) {
#pragma unroll
        for (int k = 0; k < ND; ++k) transpose4(in + 4 * k, out[0][k], out[1][k], out[2][k], out[3][k]);
    } else {
        const auto ks = std::make_integer_sequence<int, ND>{};
        channel<S, C, 0>(in, out[0], ks);
        if constexpr (C > 1) channel<S, C, 1>(in, out[1], ks);
        if constexpr (C > 2) channel<S, C, 2>(in, out[2], ks);
        if constexpr (C > 3) channel<S, C, 3>(in, out[3], ks);
    }
}

// The frame's band `band`. S: bytes a sample; C: planes, which is samples a pixel everywhere but for INDEXED (four planes, one index a pixel).
template <int S, int C>
struct Band {
    const uint8_t *s;  // the band's first source row
    uint32_t ss;       // in bytes
    uint8_t *o[C];     // the band's first row of every plane, or nullptr
    uint32_t os[C];    // in samples (32 bits each: the band's constants live in scalar registers, and those run out first)
    int rows, w;
    bool vec;          // the frame takes the unit path
    int before, after; // bytes in front of the band's first row and behind its last that are source rows, too (16 or 0; dense sources only)
    VSZIP_HD Band(const UnpackFrame &f, int band) {
        vec = f.vec != 0;
        const int y0 = band * f.rows;
        rows = f.h - y0 < f.rows ? f.h - y0 : f.rows;
        w = f.w;
        const bool dense = (long long)f.ss == (long long)f.w * C * S && C * S * f.w >= 16;  // (INDEXED does not use these two)
        before = dense && y0 > 0 ? 16 : 0;
        after = dense && y0 + rows < f.h ? 16 : 0;
        s = f.src + (size_t)y0 * (size_t)f.ss;
        ss = (uint32_t)f.ss;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            os[c] = (uint32_t)f.os[c];
            o[c] = f.o[c] ? static_cast<uint8_t *>(f.o[c]) + (size_t)y0 * os[c] * S : nullptr;
        }
    }
};

// Pixel by pixel from column x0 on: a whole frame off the unit path, or the last w % G pixels of its rows.
// mask4 / mul (S == 1 and C == 1 only): grey below 8 bits, the sample's low bits times 255 / (2^bits - 1), four samples in one multiply
// (no byte exceeds 255, so nothing carries); 8-bit grey passes 0xFFFFFFFF and 1.
template <int S, int C>
VSZIP_HD void tail_lane(const Band<S, C> &b, int x0, int tid, uint32_t mask4, uint32_t mul) {
    for_each_row_unit(tid, b.rows, b.w - x0, [&](int row, int i) {
        const size_t x = (size_t)x0 + i;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            uint32_t v = load_sample<S>(b.s + (size_t)row * b.ss + (x * C + c) * S);
            if constexpr (S == 1 && C == 1) v = (v & mask4 & 255u) * mul;
            if (b.o[c]) store_sample<S>(b.o[c] + ((size_t)row * b.os[c] + x) * S, v);
        }
    });
}

// One channel (grey): a lane loads its unit of 16 bytes straight from the source, consecutive lanes consecutive bytes.
template <int S>
VSZIP_HD void grey_lane(const UnpackFrame &f, int band, int tid, uint32_t mask4, uint32_t mul) {
    constexpr int G = 16 / S;
    const Band<S, 1> b(f, band);
    int x0 = 0;
    if (b.vec) {
        const int nv = b.w / G;
        for_each_row_unit(tid, b.rows, nv, [&](int row, int i) {
            uint32_t in[4];
            load16(in, b.s + (size_t)row * b.ss + (size_t)i * 16);
            if constexpr (S == 1) {
#pragma unroll
                for (int k = 0; k < 4; ++k) in[k] = (in[k] & mask4) * mul;
            }
            store16(b.o[0] + (size_t)row * b.os[0] * S + (size_t)i * 16, in);
        });
        x0 = nv * G;
    }
    tail_lane<S, 1>(b, x0, tid, mask4, mul);
}

// ---- several channels: the band's bytes go through LDS -----------------------------------------------------------------------------
// A lane's unit is 16 C contiguous bytes, so lanes that load their own units touch 16 bytes of every 16 C: each load instruction of a
// wave is spread over C times the lines it needs (measured: 0.58-0.67 of HBM against 0.72-0.80 this way). Instead the
// workgroup copies the bytes of a sweep, 256 units in the band's raster order, into LDS with 16-byte loads at 16-byte aligned addresses,
// consecutive lanes consecutive chunks; after the barrier a lane reads its unit from LDS as 4 C + 1 aligned dwords and shifts them by
// the source's byte phase (v_alignbyte_b32). A chunk that reaches outside the source rows is assembled from single bytes: the first and last
// chunk of every row where the pitch has padding, which is never read; where the rows are dense, the bytes around a row are its neighbours'
// and only the first chunk of a frame's first row and the last of its last row are (rows at odd bytes ran at 0.41 of HBM without this rule).
//
// A sweep holds at most 256 units: whole rows of a band whose rows are shorter (rows x units <= 256 by vszip_rows_per_workgroup),
// or 256 units of the one row of a band (units >= 256). A row's part gets a region of seg_pitch chunks: its units, up to 15 bytes
// in front (the address's phase) and the dword behind the last unit that the shift reads.
constexpr int kSweep = kThreads;
constexpr int staged_chunks(int C) { return kSweep * C + 2 * 16; }  // LDS of a workgroup, in 16-byte chunks: 16 rows at the most
VSZIP_HD int seg_pitch(int nv, int C) { return (nv < kSweep ? nv : kSweep) * C + 2; }

// (the band is built once a lane, in the kernel, and handed to every step: its constants live in scalar registers, and those run out first)
template <int S, int C>
VSZIP_HD int staged_sweeps(const Band<S, C> &b) {
    return b.vec ? (b.rows * (b.w / (16 / S)) + kSweep - 1) / kSweep : 0;
}

// before the barrier: sweep t of the band into LDS
template <int S, int C>
VSZIP_HD void stage_sweep(const Band<S, C> &b, int t, int tid, uint32_t *lds) {
    constexpr int UB = 16 * C;
    const int nv = b.w / (16 / S), total = b.rows * nv, ua = t * kSweep, ub = ua + kSweep < total ? ua + kSweep : total;
    const int r0 = ua / nv, r1 = (ub - 1) / nv, pitch = seg_pitch(nv, C);
    const size_t row_bytes = (size_t)b.w * C * S;
    for (int j = tid; j < (r1 - r0 + 1) * pitch; j += kThreads) {
        const int r = r0 + j / pitch, c = j - (r - r0) * pitch;
        const int u0 = ua > r * nv ? ua - r * nv : 0, u1 = ub < (r + 1) * nv ? ub - r * nv : nv;  // the row's units in this sweep
        const uint8_t *row = b.s + (size_t)r * b.ss, *seg = row + (size_t)u0 * UB;
        const int head = (int)(reinterpret_cast<uintptr_t>(seg) & 15), nchunk = (head + (u1 - u0) * UB + 15) / 16;
        if (c >= nchunk) continue;
        const uint8_t *p = seg - head + 16 * (size_t)c;  // a multiple of 16
        uint32_t *l = lds + ((size_t)(r - r0) * pitch + c) * 4;
        // what may be read around this row: the row, and in a dense source its neighbours as far as the band knows them to be rows
        const uint8_t *lo = row - (r > 0 ? (b.before | b.after) : b.before), *hi = row + row_bytes + (r + 1 < b.rows ? (b.before | b.after) : b.after);
        if (p >= lo && p + 16 <= hi) {
            stage16(l, p);
        } else {  // every byte from an address inside [lo, hi), the ones outside as zeros: sixteen independent loads, no branch
            uint32_t v[4] = {0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const bool in = p + k >= lo && p + k < hi;
                v[k >> 2] |= (in ? (uint32_t)*(in ? p + k : lo) : 0u) << (8 * (k & 3));
            }
            l[0] = v[0], l[1] = v[1], l[2] = v[2], l[3] = v[3];
        }
    }
}

// after the barrier: lane tid's unit of sweep t from LDS to the planes
template <int S, int C>
VSZIP_HD void unpack_sweep(const Band<S, C> &b, int t, int tid, const uint32_t *lds) {
    constexpr int UB = 16 * C, G = 16 / S, NIN = 4 * C;
    const int nv = b.w / G, total = b.rows * nv, ua = t * kSweep, j = ua + tid;
    if (j >= total) return;
    const int r0 = ua / nv, r = j / nv, i = j - r * nv, pitch = seg_pitch(nv, C);
    const int u0 = ua > r * nv ? ua - r * nv : 0;
    const int head = (int)(reinterpret_cast<uintptr_t>(b.s + (size_t)r * b.ss + (size_t)u0 * UB) & 15);
    const int off = (r - r0) * pitch * 16 + head + (i - u0) * UB;
    const uint32_t *q = lds + (off >> 2), sh = (uint32_t)off & 3u;
    uint32_t d[NIN + 1], in[NIN], out[C][4];
#pragma unroll
    for (int k = 0; k < NIN; ++k) d[k] = q[k];
    d[NIN] = sh ? q[NIN] : 0u;  // without a shift the unit ends with d[NIN - 1], and the dword behind it may lie in a chunk nobody wrote
#pragma unroll
    for (int k = 0; k < NIN; ++k) in[k] = align_byte(d[k + 1], d[k], sh);
    separate<S, C, G>(in, out);
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (b.o[c]) store16(b.o[c] + (size_t)r * b.os[c] * S + (size_t)i * 16, out[c]);
}

// and the rest of the band: the last w % G pixels of its rows, or all of it off the unit path
template <int S, int C>
VSZIP_HD void staged_tail(const Band<S, C> &b, int tid) {
    tail_lane<S, C>(b, b.vec ? b.w / (16 / S) * (16 / S) : 0, tid, ~0u, 1u);
}

// INDEXED: one index byte a pixel, tab[i] = r | g << 8 | b << 16 | a << 24 (256 dwords; LDS on the device). A unit is 16 pixels: one
// 16-byte load, sixteen gathers, and the four output bytes of four pixels assembled by transpose4.
VSZIP_HD void band_lane_indexed(const UnpackFrame &f, int band, int tid, const uint32_t *tab) {
    constexpr int G = 16;
    const Band<1, 4> b(f, band);
    int x0 = 0;
    if (b.vec) {
        const int nv = b.w / G;
        for_each_row_unit(tid, b.rows, nv, [&](int row, int i) {
            uint32_t in[4], out[4][4];
            load16(in, b.s + (size_t)row * b.ss + (size_t)i * G);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t q = in[k];
                const uint32_t t[4] = {tab[q & 255u], tab[(q >> 8) & 255u], tab[(q >> 16) & 255u], tab[q >> 24]};
                transpose4(t, out[0][k], out[1][k], out[2][k], out[3][k]);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (b.o[c]) store16(b.o[c] + (size_t)row * b.os[c] + (size_t)i * G, out[c]);
        });
        x0 = nv * G;
    }
    for_each_row_unit(tid, b.rows, b.w - x0, [&](int row, int i) {
        const size_t x = (size_t)x0 + i;
        const uint32_t t = tab[b.s[(size_t)row * b.ss + x]];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (b.o[c]) b.o[c][(size_t)row * b.os[c] + x] = (uint8_t)(t >> (8 * c));
    });
}

}  // namespace image_unpack
