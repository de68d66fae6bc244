// Stand-alone host check of vszip_color_map_lut (vapoursynth-zip_amd/csrc/host_params.cpp), built by tests/test_color_map_lut_host.py with the host
// compiler under AddressSanitizer + UndefinedBehaviorSanitizer. The palettes live in exactly sized heap blocks, so a read beyond point len - 1 is
// caught.
//   color_map_lut_check IN OUT
// IN: records of int32 len, then 3 x len f32 (r, g, b). OUT: per record int32 status, 768 table bytes (zero on an error), 128 bytes of message.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/vszip_hip.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return 2;
    int records = 0;
    int32_t len;
    while (std::fread(&len, sizeof len, 1, in) == 1) {
        const size_t n = len > 0 ? (size_t)len : 0;
        float *pal[3];
        for (int c = 0; c < 3; ++c) {
            pal[c] = new float[n ? n : 1];
            if (n && std::fread(pal[c], sizeof(float), n, in) != n) return 3;
        }
        uint8_t lut[3][256];
        std::memset(lut, 0, sizeof lut);
        char err[128];
        std::memset(err, 0, sizeof err);
        const int32_t rc = vszip_color_map_lut(pal[0], pal[1], pal[2], len, lut, err, sizeof err);
        if (rc != 0) std::memset(lut, 0, sizeof lut);
        std::fwrite(&rc, sizeof rc, 1, out);
        std::fwrite(lut, 1, sizeof lut, out);
        std::fwrite(err, 1, sizeof err, out);
        for (int c = 0; c < 3; ++c) delete[] pal[c];
        ++records;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 4;
    std::printf("%d palettes\n", records);
    return 0;
}
