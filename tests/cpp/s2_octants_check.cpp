// s2_octants_check.cpp — the S2 octant plan and the host model of S1's per-octant verdicts
// (s2_pass_count, s2_plan_octant, s2_group_walks, s2_inside_const, s2_spread, prim_interval,
// cull_one, brick_box: psgpu_model.h) compiled as plain host C++, for tests/test_s2_octants.py,
// tests/test_gpu_s2_octants.py and tools/s2_octants.py.
//
//   s2_octants_check plan
//       checks the plan for all 256 masks of decided octants and a host mirror of the bit
//       assembly of block_s2_inside_bits (psgpu_device.h) on random 512-bit patterns; prints
//       the first failures on stderr; exit code 0 only if all hold.
//   s2_octants_check <in.bin> <out.bin>
//       in.bin:  uint32 nMpus, dims[3] (the MPU lattice), bound (PSGPU_OPT_BOUND); float lo[3]
//                (the scene's bboxLo), cs; the model's device image (psgpu::DevModel,
//                psgpu_model_image); nMpus MPU origins float[3] (x-major over the lattice, as
//                the MPU ids); nMpus bytes: the MPU passed S1 (the oracle's verdict).
//       out.bin: per MPU 4 bytes: queued for S2 (passed and not proven empty), its octants
//                proven outside (bit c = xh | yh << 1 | zh << 2), proven inside, the S2 passes
//                it takes (0 if not queued).  The bits are zero without bounds (bound 0, a
//                tree that is not boundable), as on the device.
// The model is the one of cullbound_check.cpp (the tree's interval over octant_box's boxes, box-form
// intervals, the culling set of the MPU's S1 brick), kept per octant instead of per MPU, and it
// follows the generated bound() op by op, so that it also gives up (ok) exactly where that does.
#define PSGPU_MODEL_NO_HIP
#include "psgpu_model.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

using namespace psgpu;

namespace {

int g_said = 0;
#define SAY(...) do { if (g_said++ < 8) fprintf(stderr, __VA_ARGS__); } while (0)

// ---- the plan
struct Rng {  // xorshift64*
    uint64_t s;
    uint64_t next() {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        return s * 2685821657736338717ull;
    }
};

int popcount8(uint32_t v) { return __builtin_popcount(v & 0xffu); }

// The canonical layout: ins[x] bit y * 8 + z.  A pattern's bit at corner (x, y, z):
bool corner(const uint64_t ins[8], int x, int y, int z) { return (ins[x] >> (y * 8 + z)) & 1ull; }

// What a wave of block_s2_inside_bits does with a queue entry's verdicts (outside8 is only part of
// `known`) and the field's inside bits at the corners it walks (`truth`): constants first, then
// per pass the ballots of the 64 lanes' 4 points, ORed in by lanes 4g + n.
void assemble(uint32_t known, uint32_t inside8, const uint64_t truth[8], uint64_t out[8], uint32_t* walked) {
    for (int x = 0; x < 8; ++x) out[x] = s2_inside_const(inside8, (uint32_t)x >> 2);
    const uint32_t passes = s2_pass_count(known);
    for (uint32_t t = 0; t < passes; ++t) {
        uint64_t ballot[4] = {0, 0, 0, 0};
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint32_t c = s2_plan_octant(known, t, lane);
            const int y = 4 * (int)((c >> 1) & 1u) + (int)((lane >> 2) & 3u), z = 4 * (int)(c >> 2) + (int)(lane & 3u);
            for (int n = 0; n < 4; ++n)
                if (corner(truth, 4 * (int)(c & 1u) + n, y, z)) ballot[n] |= 1ull << lane;
            ++*walked;
        }
        for (uint32_t lane = 0; lane < 16; ++lane) {
            const uint32_t g16 = (lane & 12u) << 2;
            if (!s2_group_walks(known, t, g16)) continue;
            const uint32_t cg = s2_plan_octant(known, t, g16);
            out[4u * (cg & 1u) + (lane & 3u)] |= s2_spread((uint32_t)(ballot[lane & 3u] >> g16) & 0xffffu, cg);
        }
    }
}

int check_plan() {
    int bad = 0;
    Rng rng{0x9e3779b97f4a7c15ull};
    for (uint32_t known = 0; known < 256; ++known) {
        const int U = 8 - popcount8(known);
        const uint32_t passes = s2_pass_count(known);
        if ((int)passes != (U + 3) / 4) {
            ++bad;
            SAY("mask %02x: %u passes for %d undecided octants\n", known, passes, U);
        }
        int times[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        int last = -1;
        for (uint32_t t = 0; t < passes; ++t) {
            const uint32_t first = s2_plan_octant(known, t, 0);
            for (uint32_t g = 0; g < 4; ++g) {
                const uint32_t c = s2_plan_octant(known, t, 16 * g);
                for (uint32_t l = 0; l < 16; ++l)
                    if (s2_plan_octant(known, t, 16 * g + l) != c || s2_group_walks(known, t, 16 * g + l) != s2_group_walks(known, t, 16 * g)) {
                        ++bad;
                        SAY("mask %02x pass %u: lane %u differs from its group\n", known, t, 16 * g + l);
                    }
                if (c > 7 || ((known >> c) & 1u)) {
                    ++bad;
                    SAY("mask %02x pass %u group %u: walks the decided octant %u\n", known, t, g, c);
                    continue;
                }
                if (s2_group_walks(known, t, 16 * g)) {
                    ++times[c];
                    if ((int)c <= last) {
                        ++bad;
                        SAY("mask %02x pass %u group %u: octant %u out of order\n", known, t, g, c);
                    }
                    last = (int)c;
                } else if (c != first) {  // a filler repeats an octant of its own pass: the first
                    ++bad;
                    SAY("mask %02x pass %u group %u: the filler walks %u, not %u\n", known, t, g, c, first);
                }
            }
        }
        for (uint32_t c = 0; c < 8; ++c)
            if (times[c] != (((known >> c) & 1u) ? 0 : 1)) {
                ++bad;
                SAY("mask %02x: octant %u is walked %d times\n", known, c, times[c]);
            }
        // the assembly: a random pattern that agrees with the verdicts, rebuilt exactly
        for (int rep = 0; rep < 4; ++rep) {
            const uint32_t inside8 = known & (uint32_t)rng.next();
            uint64_t truth[8], got[8];
            for (int x = 0; x < 8; ++x) truth[x] = rng.next();
            for (uint32_t c = 0; c < 8; ++c) {
                if (!((known >> c) & 1u)) continue;
                const uint64_t box = 0x0f0f0f0full << (32u * ((c >> 1) & 1u) + 4u * (c >> 2));
                for (uint32_t x = 4 * (c & 1u); x < 4 * (c & 1u) + 4; ++x)
                    truth[x] = ((inside8 >> c) & 1u) ? (truth[x] | box) : (truth[x] & ~box);
            }
            uint32_t walked = 0;
            assemble(known, inside8, truth, got, &walked);
            if (memcmp(truth, got, sizeof(truth)) != 0 || walked != 64u * passes) {
                ++bad;
                SAY("mask %02x inside %02x: the assembled bits differ (%u lane walks)\n", known, inside8, walked);
            }
        }
    }
    return bad;
}

// ---- one primitive's field interval over a box as prim_bound makes it (psgpu_device.h)
struct BBox {
    float c[3], h, he[3];
};
// centre, half-diagonal and half-extents by octant_box's arithmetic (octHe: its one value)
BBox bound_box(const float lo[3], const float hi[3], float octHe) {
    BBox B;
    float hx[3];
    for (int a = 0; a < 3; ++a) {
        hx[a] = 0.5f * (hi[a] - lo[a]);
        B.c[a] = 0.5f * (lo[a] + hi[a]);
        B.he[a] = octHe;
    }
    B.h = sqrtf(hx[0] * hx[0] + hx[1] * hx[1] + hx[2] * hx[2]) * 1.0001f + 1e-4f;
    return B;
}
bool interval(const DevPrim& P, const BBox& B, float* lo, float* hi) {
    bool ok = true;
    const float hx = B.he[0], hy = B.he[1], hz = B.he[2];
    switch (P.type) {
    case PSGPU_T_POINT: prim_interval<PSGPU_T_POINT>(P, B.c[0], B.c[1], B.c[2], B.h, hx, hy, hz, lo, hi, &ok); break;
    case PSGPU_T_LINE: prim_interval<PSGPU_T_LINE>(P, B.c[0], B.c[1], B.c[2], B.h, hx, hy, hz, lo, hi, &ok); break;
    case PSGPU_T_CYLINDER: prim_interval<PSGPU_T_CYLINDER>(P, B.c[0], B.c[1], B.c[2], B.h, hx, hy, hz, lo, hi, &ok); break;
    case PSGPU_T_CUBE: prim_interval<PSGPU_T_CUBE>(P, B.c[0], B.c[1], B.c[2], B.h, hx, hy, hz, lo, hi, &ok); break;
    default: *lo = 0.0f; *hi = 0.0f; break;  // Triangle
    }
    return ok;
}

// ---- the host model of the field bounds over the walk program (bound_op, bound_prune and the
// generated bound(), psgpu_device.h / psgpu_jit.cpp): slot intervals, ops as monotone maps,
// op-box pruning of depth > 3 ops per quad of the octant
struct Oct {
    BBox B;
    float xs[4], ys[4], zs[4];
};
void op_interval(uint32_t type, float ll, float lh, float rl, float rh, float* lo, float* hi) {
    switch (type) {
    case PSGPU_T_BLEND: *lo = ll + rl; *hi = lh + rh; break;
    case PSGPU_T_UNION: *lo = fmaxf(ll, rl); *hi = fmaxf(lh, rh); break;
    case PSGPU_T_INTERSECT: *lo = fminf(ll, rl); *hi = fminf(lh, rh); break;
    case PSGPU_T_DIF: *lo = fminf(ll, 1.0f - rh); *hi = fminf(lh, 1.0f - rl); break;
    case PSGPU_T_SMOOTHDIF: {
        const float a = 1.0f - rh, b = 1.0f - rl;
        const float p0 = ll * a, p1 = ll * b, p2 = lh * a, p3 = lh * b;
        *lo = fminf(fminf(p0, p1), fminf(p2, p3));
        *hi = fmaxf(fmaxf(p0, p1), fmaxf(p2, p3));
    } break;
    default: *lo = ll; *hi = lh; break;
    }
}
void prune_interval(const DevOp& b, const Oct& O, float* lo, float* hi) {
    bool anyZ = false, allX = true, noX = true, allY = true, noY = true;
    for (int i = 0; i < 4; ++i) {
        anyZ = anyZ | ((O.zs[i] >= b.lo[2]) & (b.hi[2] >= O.zs[i]));
        const bool ix = (O.xs[i] >= b.lo[0]) & (b.hi[0] >= O.xs[i]);
        const bool iy = (O.ys[i] >= b.lo[1]) & (b.hi[1] >= O.ys[i]);
        allX = allX & ix; noX = noX & !ix;
        allY = allY & iy; noY = noY & !iy;
    }
    if (!anyZ && noX && noY) {
        *lo = 0.0f;
        *hi = 0.0f;
    } else if (!(anyZ || allX || allY)) {
        *lo = fminf(*lo, 0.0f);
        *hi = fmaxf(*hi, 0.0f);
    }
}
// The generated bound() (Gen::emit_bound_op, psgpu_jit.cpp), op by op: a subtree the culling mask
// proves +0 (zero_subtree_set) is [0, 0] and none of it is evaluated; a warp takes its left child
// and does not evaluate a primitive on its right.  What is not evaluated cannot give up (ok).
const Instr* op_instr(const DevModel& M, int op) {
    for (uint32_t k = 0; k < M.nInstr; ++k)
        if (M.instr[k].kind == kOp && M.instr[k].idx == op) return &M.instr[k];
    return nullptr;
}
void prim_bound_host(const DevModel& M, int i, const Oct& O, const bool culled[128], float* lo, float* hi, bool* ok) {
    *lo = *hi = 0.0f;
    if (i < 0 || i >= 128 || M.prims[i].type == PSGPU_T_TRIANGLE) return;
    if (prim_maybe_culled(M.prims[i]) && culled[i]) return;
    if (!interval(M.prims[i], O.B, lo, hi)) *ok = false;
}
void op_bound_host(const DevModel& M, int op, int depth, const Oct& O, const bool culled[128], float* lo, float* hi,
                   bool* ok) {
    *lo = *hi = 0.0f;
    const Instr* I = op_instr(M, op);
    if (!I || depth > 128) return;
    uint64_t m[2] = {0ull, 0ull};
    if (zero_subtree_set(M, op, m)) {
        bool zero = true;
        for (int i = 0; zero && i < 128; ++i)
            if ((m[i >> 6] >> (i & 63)) & 1ull) zero = culled[i];
        if (zero) return;
    }
    const int type = I->type, kind = I->childKind;
    const bool usesL = (type >= 14 && type <= 19) || (type >= 22 && type <= 25), usesR = type >= 14 && type <= 19;
    float ll = 0.0f, lh = 0.0f, rl = 0.0f, rh = 0.0f;
    if (kind & 1) op_bound_host(M, I->R, depth + 1, O, culled, &rl, &rh, ok);
    else if (usesR) prim_bound_host(M, I->R, O, culled, &rl, &rh, ok);
    if (kind & 2) op_bound_host(M, I->L, depth + 1, O, culled, &ll, &lh, ok);
    else if (usesL) prim_bound_host(M, I->L, O, culled, &ll, &lh, ok);
    op_interval((uint32_t)type, ll, lh, rl, rh, lo, hi);
    if (depth > 3 && op < 128) prune_interval(M.ops[op], O, lo, hi);
}
bool tree_interval(const DevModel& M, const Oct& O, const bool culled[128], float* lo, float* hi) {
    bool ok = true;
    if (M.ctOps == 0) {  // the sum of the primitives
        float sl = 0.0f, sh = 0.0f;
        for (uint32_t i = 0; i < M.ctPrims && i < 128; ++i) {
            float l, h;
            prim_bound_host(M, (int)i, O, culled, &l, &h, &ok);
            sl = sl + l;
            sh = sh + h;
        }
        *lo = sl;
        *hi = sh;
    } else {
        op_bound_host(M, 0, 0, O, culled, lo, hi, &ok);
    }
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && strcmp(argv[1], "plan") == 0) {
        const int bad = check_plan();
        if (bad) fprintf(stderr, "%d plan checks failed\n", bad);
        return bad ? 1 : 0;
    }
    if (argc != 3) {
        fprintf(stderr, "usage: %s plan | %s in.bin out.bin\n", argv[0], argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t hdr[5];
    float lo[3], cs;
    std::unique_ptr<DevModel> Mp(new DevModel);
    if (fread(hdr, 4, 5, f) != 5 || fread(lo, 4, 3, f) != 3 || fread(&cs, 4, 1, f) != 1 ||
        fread(Mp.get(), sizeof(DevModel), 1, f) != 1)
        return 3;
    const DevModel& M = *Mp;
    const uint32_t nMpus = hdr[0], dims[3] = {hdr[1], hdr[2], hdr[3]};
    const bool bound = hdr[4] != 0u && M.boundable != 0u;
    if ((uint64_t)dims[0] * dims[1] * dims[2] != nMpus) return 3;
    std::vector<float> org(3 * (size_t)nMpus);
    std::vector<uint8_t> passed(nMpus);
    if (nMpus && (fread(org.data(), 12, nMpus, f) != nMpus || fread(passed.data(), 1, nMpus, f) != nMpus)) return 3;
    fclose(f);
    const uint32_t nP = M.ctPrims < 128u ? M.ctPrims : 128u;

    std::vector<uint8_t> out(4 * (size_t)nMpus, 0);
    const float side = cs * 7.0f;
    float mag = 0.0f;
    for (int a = 0; a < 3; ++a) mag = fmaxf(mag, fmaxf(fabsf(lo[a]), fabsf(lo[a] + (float)dims[a] * side)));
    const float octHe = (1.5f * cs + 2.4e-7f * (mag + side)) * 1.0001f + 1e-4f;  // octant_box
    for (uint32_t m = 0; m < nMpus; ++m) {
        if (!passed[m]) continue;
        uint32_t out8 = 0, in8 = 0;
        if (bound) {
            const uint32_t mi = m / (dims[1] * dims[2]), mj = (m / dims[2]) % dims[1], mk = m % dims[2];
            // the culling set of the MPU's S1 wave: its brick's box (box form)
            float blo[3], bhi[3], c[3] = {0.0f, 0.0f, 0.0f}, h = 0.0f, he[3] = {0.0f, 0.0f, 0.0f};
            brick_box(lo, side, dims, mi / 2, mj / 2, mk / 2, blo, bhi);
            const bool fin = cull_box(blo[0], blo[1], blo[2], bhi[0], bhi[1], bhi[2], c, &h, he);
            bool culled[128];
            for (uint32_t i = 0; i < 128; ++i) culled[i] = fin && i < nP && cull_one(M.cull[i], c[0], c[1], c[2], h, he);
            const float* o = &org[3 * (size_t)m];
            for (int oc = 0; oc < 8; ++oc) {
                Oct O;
                for (int i = 0; i < 4; ++i) {
                    O.xs[i] = o[0] + (float)(4 * (oc & 1) + i) * cs;
                    O.ys[i] = o[1] + (float)(4 * ((oc >> 1) & 1) + i) * cs;
                    O.zs[i] = o[2] + (float)(4 * (oc >> 2) + i) * cs;
                }
                const float olo[3] = {O.xs[0], O.ys[0], O.zs[0]}, ohi[3] = {O.xs[3], O.ys[3], O.zs[3]};
                O.B = bound_box(olo, ohi, octHe);
                float l, hh;
                const bool ok = tree_interval(M, O, culled, &l, &hh);
                if (ok && hh < 0.5f) out8 |= 1u << oc;
                if (ok && l >= 0.5f) in8 |= 1u << oc;
            }
        }
        const bool queued = !(out8 == 0xffu || in8 == 0xffu);
        out[4 * (size_t)m] = queued;
        out[4 * (size_t)m + 1] = (uint8_t)out8;
        out[4 * (size_t)m + 2] = (uint8_t)in8;
        out[4 * (size_t)m + 3] = queued ? (uint8_t)s2_pass_count(out8 | in8) : 0;
    }
    f = fopen(argv[2], "wb");
    if (!f || (nMpus && fwrite(out.data(), 1, out.size(), f) != out.size())) return 5;
    fclose(f);
    return 0;
}
