// sieve_check.cpp — k_sieve's decision (psgpu::brick_box, cull_box, cull_one and the root-zero
// set, psgpu_model.h) compiled as plain host C++, for tests/test_sieve.py.
//
//   sieve_check <in.bin> <out.bin>
//
// in.bin:  float lo[3] (the scene's bboxLo), float cs, uint32 dims[3] (the MPU lattice), uint32 pad,
//          then the model's device image (psgpu::DevModel, psgpu_model_image).
// out.bin: uint32 rootZeroValid, uint32 agree (the image's root-zero set equals the one this
//          program derives from the image's walk program), uint64 rootZero[2], then one byte per
//          2x2x2 brick of the lattice, x-major: 1 if the sieve calls the brick dead.
#define PSGPU_MODEL_NO_HIP
#include "psgpu_model.h"

#include <cstdio>
#include <memory>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    float lo[3], cs;
    uint32_t dims[4];
    std::unique_ptr<psgpu::DevModel> M(new psgpu::DevModel);
    if (fread(lo, 4, 3, f) != 3 || fread(&cs, 4, 1, f) != 1 || fread(dims, 4, 4, f) != 4 ||
        fread(M.get(), sizeof(psgpu::DevModel), 1, f) != 1)
        return 3;
    fclose(f);
    const float side = cs * 7.0f;
    uint64_t mine[2];
    const bool ok = psgpu::root_zero_set(*M, mine);
    const uint32_t agree = (ok ? 1u : 0u) == M->rootZeroValid &&
                           (!ok || (mine[0] == M->rootZero[0] && mine[1] == M->rootZero[1]));
    const uint32_t nb[3] = {(dims[0] + 1) / 2, (dims[1] + 1) / 2, (dims[2] + 1) / 2};
    std::vector<uint8_t> dead((size_t)nb[0] * nb[1] * nb[2], 0);
    size_t at = 0;
    for (uint32_t bi = 0; bi < nb[0]; ++bi)
        for (uint32_t bj = 0; bj < nb[1]; ++bj)
            for (uint32_t bk = 0; bk < nb[2]; ++bk, ++at) {
                float blo[3], bhi[3], c[3], h;
                psgpu::brick_box(lo, side, dims, bi, bj, bk, blo, bhi);
                bool d = M->rootZeroValid != 0u && psgpu::cull_box(blo[0], blo[1], blo[2], bhi[0], bhi[1], bhi[2], c, &h);
                for (uint32_t i = 0; d && i < 128; ++i)
                    if ((M->rootZero[i >> 6] >> (i & 63)) & 1ull) d = psgpu::cull_one(M->cull[i], c[0], c[1], c[2], h);
                dead[at] = d ? 1 : 0;
            }
    f = fopen(argv[2], "wb");
    const uint32_t hdr[2] = {M->rootZeroValid, agree};
    if (!f || fwrite(hdr, 4, 2, f) != 2 || fwrite(M->rootZero, 8, 2, f) != 2 ||
        fwrite(dead.data(), 1, dead.size(), f) != dead.size())
        return 5;
    fclose(f);
    return 0;
}
