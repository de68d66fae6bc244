// A workgroup's lanes over a band of rows, for the streaming kernels whose planes differ in number or sample width (pack_rgb.hip,
// color_map.hip, image_unpack.hip) and so do not fit stream_map_rows of plane_table.hpp. The walk itself, the band rule and byte_perm are
// in row_walk.hpp, which is plain C++ as well.
#pragma once
#include "plane_table.hpp"
#include "row_walk.hpp"

#if defined(__HIPCC__)
// the walk of row_walk.hpp for the calling lane
template <typename F>
__device__ __forceinline__ void for_each_row_unit(int rows, int n, F f) {
    for_each_row_unit((int)threadIdx.x, rows, n, f);
}
#endif  // __HIPCC__
