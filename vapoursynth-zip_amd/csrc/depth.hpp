// vszip_depth for the entry points that run it on planes of their own (deband.hip: vszip_deband_lowbit): the carry rows a table of
// conversions takes from the caller's scratch layout, and the launches themselves.
#pragma once
#include <vector>

#include "common.hpp"
#include "depth_plan.hpp"

// the workgroup (in waves) a plane of h rows takes under the context's VSZIP_DEPTH_WAVES
int vszip_depth_waves(const vszip_ctx *ctx, int h);
// one region per plane, in order: w floats for an error-diffusion plane whose carry row leaves LDS, else empty
void vszip_depth_take_carry(const vszip_ctx *ctx, scratch::Layout &lay, const vszip_depth_plane *planes, int nplanes, int dither,
                            std::vector<scratch::Region<float>> &carry);
// queues the conversions (arguments already checked by vszip_depth_check); carry / base: the regions above in the reserved scratch
int vszip_depth_queue(vszip_ctx *ctx, const vszip_depth_plane *planes, int nplanes, int bits_in, int bits_out, int dither, int full_range,
                      const std::vector<scratch::Region<float>> &carry, char *base);
