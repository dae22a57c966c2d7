// divby_check.cpp — psgpu::div_by (psgpu_model.h: the exact m / d behind mpu_origin, the S1 brick
// decode and k_sieve's) compiled as plain host C++, for tests/test_aniso.py.
//
//   divby_check <out.bin> [d0 d1 d2]...
//
// 1. Every d in 1..4096 and d = 2^16 - 1, 2^16, 2^16 + 1, 2^21, 2^31, 2^32 - 1, with
//    magic = 0xffffffff / d as the host sets it: quotient and remainder equal / and % at
//    m = 0, 1, d - 1, d, d + 1, every k * d - 1 and k * d for k up to 64, 2^31 - 1, 2^31 + 1,
//    2^32 - d, 2^32 - 1 and 10^5 seeded random values.
// 2. For every MPU lattice (d0, d1, d2) of the command line: mpu_origin's decode of every MPU
//    id, and precheck_body's / k_sieve's decode of every brick id of the lattice's
//    ((d + 1) / 2 per axis) bricks, each as (i, jk, j, k), against / and %.  The decoded
//    (i, j, k) go to out.bin as uint32 triples, MPUs first, then bricks, lattice after lattice.
// Prints the number of checks; exit code 1 and the first mismatch on stderr otherwise.
#define PSGPU_MODEL_NO_HIP
#include "psgpu_model.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static unsigned long long g_checks = 0;

static bool check(uint32_t m, uint32_t d) {
    const uint32_t magic = 0xffffffffu / d;
    uint32_t r = 0xdeadbeefu;
    const uint32_t q = psgpu::div_by(m, d, magic, &r);
    ++g_checks;
    if (q == m / d && r == m % d) return true;
    fprintf(stderr, "div_by(%u, %u): got %u rem %u, want %u rem %u\n", m, d, q, r, m / d, m % d);
    return false;
}

static bool check_d(uint32_t d) {
    const uint32_t edge[] = {0u, 1u, d - 1u, d, d + 1u, 0x7fffffffu, 0x80000001u, 0u - d, 0xffffffffu};
    for (uint32_t m : edge)
        if (!check(m, d)) return false;
    for (uint64_t k = 1; k <= 64 && k * d <= 0xffffffffull; ++k)
        if (!check((uint32_t)(k * d - 1u), d) || !check((uint32_t)(k * d), d)) return false;
    const uint64_t span = (uint64_t)d << 21;
    uint64_t s = 0x9e3779b97f4a7c15ull * (d + 1ull);  // splitmix64, seeded by d
    for (int i = 0; i < 100000; ++i) {
        s += 0x9e3779b97f4a7c15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        // every other value below 2^21 * d: the quotients a lattice decode meets
        const uint32_t m = (i & 1) ? (uint32_t)z : (uint32_t)(z % (span < 0x100000000ull ? span : 0x100000000ull));
        if (!check(m, d)) return false;
    }
    return true;
}

// the decode of id b over a (ny, nz) cross-section, as mpu_origin and precheck_body write it
static bool decode(uint32_t b, uint32_t ny, uint32_t nz, std::vector<uint32_t>& out) {
    const uint32_t magic[2] = {0xffffffffu / nz, 0xffffffffu / (ny * nz)};
    uint32_t jk, k;
    const uint32_t i = psgpu::div_by(b, ny * nz, magic[1], &jk);
    const uint32_t j = psgpu::div_by(jk, nz, magic[0], &k);
    ++g_checks;
    if (i != b / (ny * nz) || jk != b % (ny * nz) || j != (b % (ny * nz)) / nz || k != b % nz) {
        fprintf(stderr, "decode(%u over %u x %u): got i %u jk %u j %u k %u\n", b, ny, nz, i, jk, j, k);
        return false;
    }
    out.push_back(i);
    out.push_back(j);
    out.push_back(k);
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2 || (argc - 2) % 3 != 0) {
        fprintf(stderr, "usage: %s out.bin [d0 d1 d2]...\n", argv[0]);
        return 2;
    }
    for (uint32_t d = 1; d <= 4096u; ++d)
        if (!check_d(d)) return 1;
    const uint32_t wide[] = {0xffffu, 0x10000u, 0x10001u, 1u << 21, 1u << 31, 0xffffffffu};
    for (uint32_t d : wide)
        if (!check_d(d)) return 1;
    std::vector<uint32_t> out;
    for (int a = 2; a + 2 < argc; a += 3) {
        const uint32_t dims[3] = {(uint32_t)atoi(argv[a]), (uint32_t)atoi(argv[a + 1]), (uint32_t)atoi(argv[a + 2])};
        if (!dims[0] || !dims[1] || !dims[2]) return 2;
        for (uint32_t m = 0; m < dims[0] * dims[1] * dims[2]; ++m)
            if (!decode(m, dims[1], dims[2], out)) return 1;
        const uint32_t nb[3] = {(dims[0] + 1) / 2, (dims[1] + 1) / 2, (dims[2] + 1) / 2};
        for (uint32_t b = 0; b < nb[0] * nb[1] * nb[2]; ++b)
            if (!decode(b, nb[1], nb[2], out)) return 1;
    }
    FILE* f = fopen(argv[1], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return 5;
    fclose(f);
    printf("%llu checks\n", g_checks);
    return 0;
}
