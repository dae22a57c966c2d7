// op_inside_check.cpp — the op-inside mask predicate (psgpu::op_inside_box, psgpu_model.h)
// compiled as plain host C++, for tests/test_op_inside.py.
//
//   op_inside_check <in.bin> <out.bin>
//
// in.bin:  uint32 nOps, uint32 nMpus, float cs, uint32 pad; nOps x {lo[3], hi[3]} floats (the ops'
//          vBoxLo / vBoxHi); nMpus x float[3] MPU origins.
// out.bin: nMpus x 2 uint64: bit k of the pair set when op k's predicate holds for the MPU, as
//          k_precheck's ballots lay the bits out (psgpu_device.h, precheck_body).
#define PSGPU_MODEL_NO_HIP
#include "psgpu_model.h"

#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t hdr[4];
    float cs;
    if (fread(hdr, 4, 4, f) != 4) return 3;
    __builtin_memcpy(&cs, &hdr[2], 4);
    const uint32_t nOps = hdr[0], nMpus = hdr[1];
    if (nOps > 128) return 4;
    std::vector<float> ops(6 * (size_t)nOps), org(3 * (size_t)nMpus);
    if (fread(ops.data(), 4, ops.size(), f) != ops.size() || fread(org.data(), 4, org.size(), f) != org.size()) return 3;
    fclose(f);
    std::vector<uint64_t> out(2 * (size_t)nMpus, 0ull);
    for (uint32_t w = 0; w < nMpus; ++w)
        for (uint32_t k = 0; k < nOps; ++k)
            if (psgpu::op_inside_box(&ops[6 * k], &ops[6 * k + 3], org[3 * w], org[3 * w + 1], org[3 * w + 2], cs))
                out[2 * w + (k >> 6)] |= 1ull << (k & 63);
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 8, out.size(), f) != out.size()) return 5;
    fclose(f);
    return 0;
}
