// cullbound_check.cpp — the box bounds of the culling masks and of the S1 field proofs
// (psgpu::cull_box, cull_one, prim_interval: psgpu_model.h) compiled as plain host C++, for
// tests/test_cullbound.py and tools/cull_pairs.py.
//
//   cullbound_check <in.bin> <out.bin>
//
// in.bin:  uint32 nBoxes, nMpus, dims[3] (the MPU lattice), seed; float lo[3] (the scene's
//          bboxLo), cs; the model's device image (psgpu::DevModel, psgpu_model_image); then
//          nBoxes boxes float[6] = {x0, y0, z0, x1, y1, z1}; then nMpus MPU origins float[3]
//          (x-major over the lattice, as the MPU ids).
// out.bin: uint64 box[8]: (box, primitive) pairs tested, culled by the sphere form, culled by
//          the box form, culled pairs with a sample point of dist2 < 1, pairs the sphere form
//          culls and the box form does not, intervals tested, intervals that miss a sample's
//          field, intervals wider than the sphere form's;
//          uint64 pairs[2][2][5]: live (box, primitive) pairs over [MPU boxes, S1 brick boxes] x
//          [sphere form, box form] x [all, Cube, Point, Cylinder, Line];
//          uint64 deadBricks[2]: bricks without a live primitive, sphere and box form;
//          then per MPU 4 bytes: every primitive of the root-zero set is culled over the MPU's
//          box (sphere form, box form); the host model of the field bounds proves it empty
//          (sphere-form interval, box-form interval).
// The first few failures are described on stderr.  The exit code says only that the files
// were read and written: the test asserts on the counts.
#define PSGPU_MODEL_NO_HIP
#include "psgpu_model.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

using namespace psgpu;

namespace {

// ---- the reference's fp32 formulas, in its operation order (computePrimitiveField,
// PS_Polygonizer.cpp:975-1097; the same expressions as prim_dist2 / wyvill, psgpu_device.h)
float max_ref(float a, float b) { return a > b ? a : b; }
float m01(bool c) { return c ? 1.0f : 0.0f; }

float ref_dist2(const DevPrim& P, float x, float y, float z) {
    float d2 = 0.0f;
    if (P.type == PSGPU_T_POINT) {
        float dx = P.pos[0] - x, dy = P.pos[1] - y, dz = P.pos[2] - z;
        d2 = (dx * dx + dy * dy) + dz * dz;
    } else if (P.type == PSGPU_T_LINE) {
        float l0x = P.pos[0], l0y = P.pos[1], l0z = P.pos[2];
        float ldx = P.dir[0] - l0x, ldy = P.dir[1] - l0y, ldz = P.dir[2] - l0z;
        float ldd = (ldx * ldx + ldy * ldy) + ldz * ldz;
        float dx = x - l0x, dy = y - l0y, dz = z - l0z;
        float t = (dx * ldx + dy * ldy) + dz * ldz;
        t = t / ldd;
        dx = x - (l0x + t * ldx);
        dy = y - (l0y + t * ldy);
        dz = z - (l0z + t * ldz);
        d2 = (dx * dx + dy * dy) + dz * dz;
    } else if (P.type == PSGPU_T_CYLINDER) {
        float px = x - P.pos[0], py = y - P.pos[1], pz = z - P.pos[2];
        float yy = (px * P.dir[0] + py * P.dir[1]) + pz * P.dir[2];
        float rr = ((px * px + py * py) + pz * pz) - yy * yy;
        float xx = max_ref(0.0f, sqrtf(rr) - P.res[0]);
        float mask = m01(yy > 0.0f);
        yy = mask * max_ref(0.0f, yy - P.res[1]) + (1.0f - mask) * yy;
        d2 = xx * xx + yy * yy;
    } else if (P.type == PSGPU_T_TRIANGLE) {
        d2 = 3.402823466e+38f;
    } else if (P.type == PSGPU_T_CUBE) {
        float side = P.res[0], mside = -1.0f * P.res[0];
        float dif[3] = {x - P.pos[0], y - P.pos[1], z - P.pos[2]};
        for (int a = 0; a < 3; ++a) {
            float mm = m01(mside > dif[a]);
            float mp = m01(dif[a] > side);
            float dl = (dif[a] + side) * mm + (dif[a] - side) * mp;
            d2 = (a == 0) ? dl * dl : d2 + dl * dl;
        }
    }
    return d2;
}

float ref_wyvill(float d2) {
    float t = 1.0f - d2;
    float f = (t * t) * t;
    return max_ref(0.0f, f);
}

// ---- boxes
struct Box {
    float lo[3], hi[3];
};

float clampf(float v, float a, float b) { return v < a ? a : (v > b ? b : v); }

// The point of the primitive nearest q (double: only to place a sample point)
void nearest_on_prim(const DevPrim& P, const double q[3], double out[3]) {
    if (P.type == PSGPU_T_LINE || P.type == PSGPU_T_CYLINDER) {
        double u[3], d[3], uu = 0.0, du = 0.0;
        for (int a = 0; a < 3; ++a) {
            u[a] = P.type == PSGPU_T_LINE ? (double)P.dir[a] - P.pos[a] : (double)P.dir[a];
            d[a] = q[a] - P.pos[a];
            uu += u[a] * u[a];
            du += d[a] * u[a];
        }
        double t = uu > 0.0 ? du / uu : 0.0;
        if (P.type == PSGPU_T_CYLINDER) {
            const double len = std::sqrt(uu);
            const double y = len > 0.0 ? du / len : 0.0, yc = y < 0.0 ? 0.0 : (y > P.res[1] ? (double)P.res[1] : y);
            double r[3], rn = 0.0;
            for (int a = 0; a < 3; ++a) {
                r[a] = d[a] - (len > 0.0 ? y * u[a] / len : 0.0);
                rn += r[a] * r[a];
            }
            rn = std::sqrt(rn);
            const double k = rn > P.res[0] ? P.res[0] / rn : 1.0;
            for (int a = 0; a < 3; ++a) out[a] = P.pos[a] + (len > 0.0 ? yc * u[a] / len : 0.0) + k * r[a];
            return;
        }
        for (int a = 0; a < 3; ++a) out[a] = P.pos[a] + t * u[a];
    } else if (P.type == PSGPU_T_CUBE) {
        for (int a = 0; a < 3; ++a) {
            const double l = (double)P.pos[a] - P.res[0], h = (double)P.pos[a] + P.res[0];
            out[a] = q[a] < l ? l : (q[a] > h ? h : q[a]);
        }
    } else {
        for (int a = 0; a < 3; ++a) out[a] = P.pos[a];
    }
}

struct Rng {  // xorshift64*
    uint64_t s;
    float unit() {
        s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
        return (float)((s * 2685821657736338717ull) >> 40) * (1.0f / 16777216.0f);
    }
};

// Sample points of a box: corners, centre, face centres, the box point nearest the primitive
// (alternating projections), 64 random points.  All inside the box as fp32 values.
int sample_points(const Box& B, const DevPrim& P, Rng& rng, float pts[96][3]) {
    int n = 0;
    const float c[3] = {clampf(0.5f * (B.lo[0] + B.hi[0]), B.lo[0], B.hi[0]), clampf(0.5f * (B.lo[1] + B.hi[1]), B.lo[1], B.hi[1]),
                        clampf(0.5f * (B.lo[2] + B.hi[2]), B.lo[2], B.hi[2])};
    for (int k = 0; k < 8; ++k, ++n)
        for (int a = 0; a < 3; ++a) pts[n][a] = ((k >> a) & 1) ? B.hi[a] : B.lo[a];
    for (int a = 0; a < 3; ++a) pts[n][a] = c[a];
    ++n;
    for (int f = 0; f < 6; ++f, ++n)
        for (int a = 0; a < 3; ++a) pts[n][a] = a == f / 2 ? ((f & 1) ? B.hi[a] : B.lo[a]) : c[a];
    double q[3] = {c[0], c[1], c[2]}, pk[3];
    for (int it = 0; it < 6; ++it) {
        nearest_on_prim(P, q, pk);
        for (int a = 0; a < 3; ++a) q[a] = pk[a] < B.lo[a] ? B.lo[a] : (pk[a] > B.hi[a] ? B.hi[a] : pk[a]);
    }
    for (int a = 0; a < 3; ++a) pts[n][a] = clampf((float)q[a], B.lo[a], B.hi[a]);
    ++n;
    for (int k = 0; k < 64; ++k, ++n)
        for (int a = 0; a < 3; ++a) pts[n][a] = clampf(B.lo[a] + rng.unit() * (B.hi[a] - B.lo[a]), B.lo[a], B.hi[a]);
    return n;
}

// ---- one primitive's field interval over a box as prim_bound makes it (psgpu_device.h), and the
// sphere form alone (hx = hy = hz = +inf leaves only d - h and d + h of prim_interval)
struct BBox {
    float c[3], h, he[3];
};
// centre and half-diagonal by octant_box's arithmetic; the half-extents with the same slack,
// per axis from the box (any box), or octant_box's one value for the lattice's octants
BBox bound_box(const float lo[3], const float hi[3], float octHe = 0.0f) {
    BBox B;
    float hx[3];
    for (int a = 0; a < 3; ++a) {
        hx[a] = 0.5f * (hi[a] - lo[a]);
        B.c[a] = 0.5f * (lo[a] + hi[a]);
    }
    B.h = sqrtf(hx[0] * hx[0] + hx[1] * hx[1] + hx[2] * hx[2]) * 1.0001f + 1e-4f;
    for (int a = 0; a < 3; ++a)
        B.he[a] = octHe > 0.0f ? octHe : box_half_extent(lo[a], hi[a], B.c[a]) * 1.0001f + 1e-4f;
    return B;
}
bool interval(const DevPrim& P, const BBox& B, bool tight, float* lo, float* hi) {
    bool ok = true;
    const float inf = __builtin_inff();
    const float hx = tight ? B.he[0] : inf, hy = tight ? B.he[1] : inf, hz = tight ? B.he[2] : inf;
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
void op_depths(const DevModel& M, int op, int depth, int out[128]) {
    if (op < 0 || op >= 128 || depth > 128) return;
    out[op] = depth;
    for (uint32_t k = 0; k < M.nInstr; ++k)
        if (M.instr[k].kind == kOp && M.instr[k].idx == op) {
            if (M.instr[k].childKind & 2) op_depths(M, M.instr[k].L, depth + 1, out);
            if (M.instr[k].childKind & 1) op_depths(M, M.instr[k].R, depth + 1, out);
            return;
        }
}
bool tree_interval(const DevModel& M, const int depth[128], const Oct& O, const bool culled[128], bool tight, float* lo,
                   float* hi) {
    float sl[kMaxSlots], sh[kMaxSlots], accL = 0.0f, accH = 0.0f, lastL = 0.0f, lastH = 0.0f;
    memset(sl, 0, sizeof(sl));
    memset(sh, 0, sizeof(sh));
    bool ok = true;
    for (uint32_t pc = 0; pc < M.nInstr; ++pc) {
        const Instr& I = M.instr[pc];
        if (I.kind == kPrim || I.kind == kSumPrim) {
            float l = 0.0f, h = 0.0f;
            if (I.idx < 128 && !culled[I.idx]) ok = interval(M.prims[I.idx], O.B, tight, &l, &h) && ok;
            if (I.kind == kSumPrim) {
                accL += l;
                accH += h;
            } else {
                sl[I.out % kMaxSlots] = l;
                sh[I.out % kMaxSlots] = h;
            }
        } else if (I.kind == kOp) {
            float l, h;
            op_interval(I.type, sl[I.lslot % kMaxSlots], sh[I.lslot % kMaxSlots], sl[I.rslot % kMaxSlots],
                        sh[I.rslot % kMaxSlots], &l, &h);
            if (I.idx < 128 && depth[I.idx] > 3) prune_interval(M.ops[I.idx], O, &l, &h);
            sl[I.out % kMaxSlots] = lastL = l;
            sh[I.out % kMaxSlots] = lastH = h;
        }
    }
    *lo = M.ctOps == 0 ? accL : lastL;
    *hi = M.ctOps == 0 ? accH : lastH;
    return ok;
}

int type_column(uint32_t t) {
    return t == PSGPU_T_CUBE ? 1 : t == PSGPU_T_POINT ? 2 : t == PSGPU_T_CYLINDER ? 3 : t == PSGPU_T_LINE ? 4 : -1;
}

int g_said = 0;
#define SAY(...) do { if (g_said++ < 8) fprintf(stderr, __VA_ARGS__); } while (0)

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t hdr[6];
    float lo[3], cs;
    std::unique_ptr<DevModel> Mp(new DevModel);
    if (fread(hdr, 4, 6, f) != 6 || fread(lo, 4, 3, f) != 3 || fread(&cs, 4, 1, f) != 1 ||
        fread(Mp.get(), sizeof(DevModel), 1, f) != 1)
        return 3;
    const DevModel& M = *Mp;
    const uint32_t nBoxes = hdr[0], nMpus = hdr[1], dims[3] = {hdr[2], hdr[3], hdr[4]};
    std::vector<Box> boxes(nBoxes);
    std::vector<float> org(3 * (size_t)nMpus);
    if ((nBoxes && fread(boxes.data(), sizeof(Box), nBoxes, f) != nBoxes) ||
        (nMpus && fread(org.data(), 12, nMpus, f) != nMpus))
        return 3;
    fclose(f);
    Rng rng{0x9e3779b97f4a7c15ull ^ ((uint64_t)hdr[5] << 17) ^ 1ull};
    const uint32_t nP = M.ctPrims < 128u ? M.ctPrims : 128u;

    // ---- every (box, primitive) pair of the list
    uint64_t box[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float pts[96][3];
    for (uint32_t b = 0; b < nBoxes; ++b) {
        const Box& B = boxes[b];
        float c[3], h, he[3], c0[3], h0;
        const bool fin = cull_box(B.lo[0], B.lo[1], B.lo[2], B.hi[0], B.hi[1], B.hi[2], c, &h, he);
        const bool fin0 = cull_box(B.lo[0], B.lo[1], B.lo[2], B.hi[0], B.hi[1], B.hi[2], c0, &h0);
        const BBox BB = bound_box(B.lo, B.hi);
        for (uint32_t i = 0; i < nP; ++i) {
            const DevPrim& P = M.prims[i];
            const bool was = fin0 && cull_one(M.cull[i], c0[0], c0[1], c0[2], h0);
            const bool now = fin && cull_one(M.cull[i], c[0], c[1], c[2], h, he);
            ++box[0];
            box[1] += was;
            box[2] += now;
            if (was && !now) {
                ++box[4];
                SAY("box %u prim %u (type %u): the sphere form culls it, the box form does not\n", b, i, P.type);
            }
            const bool bounded = (P.cullable & 1u) != 0u;
            if (!now && !bounded) continue;
            const int n = sample_points(B, P, rng, pts);
            if (now) {
                bool bad = false;
                for (int k = 0; k < n && !bad; ++k) {
                    const float d2 = ref_dist2(P, pts[k][0], pts[k][1], pts[k][2]);
                    if (!(d2 >= 1.0f)) {
                        bad = true;
                        SAY("box %u prim %u (type %u): culled, but dist2 = %.9g at (%.9g, %.9g, %.9g)\n", b, i, P.type, d2,
                            pts[k][0], pts[k][1], pts[k][2]);
                    }
                }
                box[3] += bad;
            }
            if (bounded && fin) {
                float l0, h0i, l1, h1;
                const bool ok0 = interval(P, BB, false, &l0, &h0i), ok1 = interval(P, BB, true, &l1, &h1);
                if (!ok1) continue;
                ++box[5];
                if (ok0 && (l1 < l0 || h1 > h0i)) {
                    ++box[7];
                    SAY("box %u prim %u (type %u): [%.9g, %.9g] is wider than the sphere form's [%.9g, %.9g]\n", b, i,
                        P.type, l1, h1, l0, h0i);
                }
                bool bad = false;
                for (int k = 0; k < n && !bad; ++k) {
                    const float fv = ref_wyvill(ref_dist2(P, pts[k][0], pts[k][1], pts[k][2]));
                    if (!(fv >= l1 && fv <= h1)) {
                        bad = true;
                        SAY("box %u prim %u (type %u): field %.9g at (%.9g, %.9g, %.9g) outside [%.9g, %.9g]\n", b, i, P.type,
                            fv, pts[k][0], pts[k][1], pts[k][2], l1, h1);
                    }
                }
                box[6] += bad;
            }
        }
    }

    // ---- the lattice: live pairs over MPU boxes and S1 brick boxes, and the two verdicts per MPU
    uint64_t pairs[2][2][5];
    uint64_t deadBricks[2] = {0, 0};
    memset(pairs, 0, sizeof(pairs));
    std::vector<uint8_t> verdict(4 * (size_t)nMpus, 0);
    const float side = cs * 7.0f, eg = 7.0f * cs + 0.001f;
    float mag = 0.0f;
    for (int a = 0; a < 3; ++a) mag = fmaxf(mag, fmaxf(fabsf(lo[a]), fabsf(lo[a] + (float)dims[a] * side)));
    const float octHe = (1.5f * cs + 2.4e-7f * (mag + side)) * 1.0001f + 1e-4f;  // octant_box
    auto masks = [&](const float blo[3], const float bhi[3], bool culled[2][128], int where) {
        float c[3], h, he[3];
        const bool fin = cull_box(blo[0], blo[1], blo[2], bhi[0], bhi[1], bhi[2], c, &h, he);
        for (uint32_t i = 0; i < 128; ++i) {
            culled[0][i] = fin && i < nP && cull_one(M.cull[i], c[0], c[1], c[2], h);
            culled[1][i] = fin && i < nP && cull_one(M.cull[i], c[0], c[1], c[2], h, he);
            const int col = type_column(M.prims[i].type);
            for (int v = 0; v < 2 && i < nP; ++v)
                if (!culled[v][i]) {
                    ++pairs[where][v][0];
                    if (col > 0) ++pairs[where][v][col];
                }
        }
    };
    if (nMpus) {
        int depth[128];
        memset(depth, 0, sizeof(depth));
        if (M.ctOps) op_depths(M, 0, 0, depth);
        const uint32_t nb[3] = {(dims[0] + 1) / 2, (dims[1] + 1) / 2, (dims[2] + 1) / 2};
        std::vector<bool> brickCulled[2];  // per brick and version, 128 flags
        brickCulled[0].resize((size_t)nb[0] * nb[1] * nb[2] * 128);
        brickCulled[1].resize(brickCulled[0].size());
        size_t at = 0;
        bool culled[2][128];
        for (uint32_t bi = 0; bi < nb[0]; ++bi)
            for (uint32_t bj = 0; bj < nb[1]; ++bj)
                for (uint32_t bk = 0; bk < nb[2]; ++bk, ++at) {
                    float blo[3], bhi[3];
                    brick_box(lo, side, dims, bi, bj, bk, blo, bhi);
                    masks(blo, bhi, culled, 1);
                    for (int v = 0; v < 2; ++v) {
                        bool any = false;
                        for (uint32_t i = 0; i < 128; ++i) {
                            brickCulled[v][at * 128 + i] = culled[v][i];
                            any = any || (i < nP && !culled[v][i]);
                        }
                        deadBricks[v] += !any;
                    }
                }
        for (uint32_t m = 0; m < nMpus; ++m) {
            const float* o = &org[3 * (size_t)m];
            const float mlo[3] = {o[0], o[1], o[2]}, mhi[3] = {o[0] + eg, o[1] + eg, o[2] + eg};
            masks(mlo, mhi, culled, 0);
            for (int v = 0; v < 2; ++v) {
                bool zero = M.rootZeroValid != 0u;
                for (uint32_t i = 0; zero && i < 128; ++i)
                    if ((M.rootZero[i >> 6] >> (i & 63)) & 1ull) zero = culled[v][i];
                verdict[4 * (size_t)m + v] = zero;
            }
            if (!M.boundable) continue;
            const uint32_t mi = m / (dims[1] * dims[2]), mj = (m / dims[2]) % dims[1], mk = m % dims[2];
            const size_t brick = ((size_t)(mi / 2) * nb[1] + mj / 2) * nb[2] + mk / 2;
            for (int v = 0; v < 2; ++v) {
                bool bc[128];
                for (uint32_t i = 0; i < 128; ++i) bc[i] = brickCulled[v][brick * 128 + i];
                bool allOut = true, allIn = true;
                for (int c = 0; c < 8; ++c) {
                    Oct O;
                    for (int i = 0; i < 4; ++i) {
                        O.xs[i] = o[0] + (float)(4 * (c & 1) + i) * cs;
                        O.ys[i] = o[1] + (float)(4 * ((c >> 1) & 1) + i) * cs;
                        O.zs[i] = o[2] + (float)(4 * (c >> 2) + i) * cs;
                    }
                    const float olo[3] = {O.xs[0], O.ys[0], O.zs[0]}, ohi[3] = {O.xs[3], O.ys[3], O.zs[3]};
                    O.B = bound_box(olo, ohi, octHe);
                    float l, h;
                    const bool ok = tree_interval(M, depth, O, bc, v == 1, &l, &h);
                    allOut = allOut && ok && h < 0.5f;
                    allIn = allIn && ok && l >= 0.5f;
                }
                verdict[4 * (size_t)m + 2 + v] = allOut || allIn;
            }
        }
    }

    f = fopen(argv[2], "wb");
    if (!f || fwrite(box, 8, 8, f) != 8 || fwrite(pairs, 8, 20, f) != 20 || fwrite(deadBricks, 8, 2, f) != 2 ||
        (nMpus && fwrite(verdict.data(), 1, verdict.size(), f) != verdict.size()))
        return 5;
    fclose(f);
    return 0;
}
