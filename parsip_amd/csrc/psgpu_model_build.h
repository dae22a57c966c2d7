// psgpu_model_build.h — a caller's SoA model into what the device reads, on the host alone.
//
// The walk program and the 28 KB DevModel image (build_device_model), the MPU lattice
// (lattice_dims), PrepareBBoxes, the BlobTree type map and the cost split: pure arithmetic over
// caller-supplied bytes, with no context and no HIP call.  This is the code that decides which
// caller-supplied trees the device walk may dereference, and every byte of the image matters
// (set_model compares images with memcmp; the graph key and the JIT cache hang off them).
// psgpu_host.cpp's entry points forward here.
//
// Host only, and not embedded for hiprtc.  A plain C++ program (tests/cpp/model_build_check.cpp)
// defines PSGPU_MODEL_NO_HIP first and needs no ROCm headers.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/parsip_gpu.h"
#include "psgpu_model.h"

namespace psgpu {

// ---------------------------------------------------------------------------
// Walk program: the reference's processing order of fieldValue's explicit stack.
inline bool op_needs_left(int t) { return (t >= 14 && t <= 19) || (t >= 22 && t <= 25); }
inline bool op_needs_right(int t) { return t >= 14 && t <= 19; }

struct ProgramBuilder {
    const PsSoaBlobOps& O;
    std::vector<Instr> prog;
    std::vector<uint8_t> seen;
    int maxSlot = 0;
    bool ok = true;

    explicit ProgramBuilder(const PsSoaBlobOps& ops) : O(ops), seen(128, 0) {}

    void emit(int op, int depth, int h) {
        if (!ok) return;
        if (op < 0 || op >= (int)O.ctOps || seen[op] || depth > 127 || h + 3 >= kMaxSlots) {
            ok = false;
            return;
        }
        seen[op] = 1;
        const int kind = O.opChildKind[op];
        const int L = O.opLeftChild[op], R = O.opRightChild[op];
        const int type = O.opType[op];
        size_t enterAt = 0;
        if (depth > 3) {
            Instr e{};
            e.kind = kEnter;
            e.idx = (uint16_t)op;
            e.out = (uint8_t)h;
            enterAt = prog.size();
            prog.push_back(e);
        }
        int next = h, lslot = 0, rslot = 0;
        if (kind & 1) {  // right op subtree first (pushed last, popped first)
            emit(R, depth + 1, h);
            rslot = h;
            next = h + 1;
        }
        if (kind & 2) {
            emit(L, depth + 1, next);
            lslot = next;
            next = next + 1;
        }
        if (!ok) return;
        int freeSlot = next;
        if (!(kind & 2) && op_needs_left(type)) {
            if (L >= 128) { ok = false; return; }
            Instr p{};
            p.kind = kPrim;
            p.idx = (uint16_t)L;
            p.out = (uint8_t)freeSlot;
            prog.push_back(p);
            lslot = freeSlot++;
        }
        if (!(kind & 1) && op_needs_right(type)) {
            if (R >= 128) { ok = false; return; }
            Instr p{};
            p.kind = kPrim;
            p.idx = (uint16_t)R;
            p.out = (uint8_t)freeSlot;
            prog.push_back(p);
            rslot = freeSlot++;
        }
        maxSlot = std::max(maxSlot, freeSlot);
        Instr c{};
        c.kind = kOp;
        c.type = (uint8_t)type;
        c.out = (uint8_t)h;
        c.lslot = (uint8_t)lslot;
        c.rslot = (uint8_t)rslot;
        c.childKind = (uint8_t)kind;
        c.L = (uint8_t)L;
        c.R = (uint8_t)R;
        c.idx = (uint16_t)op;
        prog.push_back(c);
        if (depth > 3) prog[enterAt].skipTo = (uint16_t)prog.size();
        if (prog.size() > (size_t)kMaxInstr) ok = false;
    }
};

inline bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// Colour of op `op` when its subtree is all +0 fields (culled primitives, or pruned: the
// reference's colour pass then reads zeroed arrays, :1472-1522): a constant of the tree and the
// primitive colours, computed in fp32 exactly as op_colour_weights + the weighted sum on the
// device.  Children first (post-order over the tree the program builder validated: every child op
// id < ctOps, no cycles), so any op numbering works, not only pre-order.
// A primitive child id is validated (< 128) only under an op type that evaluates that side; under
// any other type an id up to 255 reads pc[k][id], at most colorZ[255]: past its array but inside
// PsSoaBlobPrims (the box arrays follow the colours), and the value read only reaches a zeroCol
// entry that no walk uses.  The bytes are kept as they were.
inline void zero_col(const PsSoaBlobOps& O, const float* const pc[3], DevModel& D, int op) {
    const uint32_t t = O.opType[op], kind = O.opChildKind[op];
    const uint32_t L = O.opLeftChild[op], R = O.opRightChild[op];
    if (kind & 2) zero_col(O, pc, D, (int)L);
    if (kind & 1) zero_col(O, pc, D, (int)R);
    float cl[3], cr[3];
    for (int k = 0; k < 3; ++k) {
        cl[k] = (kind & 2) ? D.zeroCol[L][k] : pc[k][L];
        cr[k] = (kind & 1) ? D.zeroCol[R][k] : pc[k][R];
    }
    const float lf = 0.0f, rf = 0.0f;
    float v = 0.0f, wl = 0.0f, wr = 0.0f;
    bool weighted = true;
    switch (t) {
    case PSGPU_OP_BLEND: v = lf + rf; wl = 2.0f * (0.5f + lf) - 1.0f; wr = 2.0f * (0.5f + rf) - 1.0f; break;
    case PSGPU_OP_UNION: v = lf > rf ? lf : rf; wl = (v - lf) == 0.0f ? 1.0f : 0.0f; wr = (v - rf) == 0.0f ? 1.0f : 0.0f; break;
    case PSGPU_OP_INTERSECT: v = lf < rf ? lf : rf; wl = (v - lf) == 0.0f ? 1.0f : 0.0f; wr = (v - rf) == 0.0f ? 1.0f : 0.0f; break;
    case PSGPU_OP_DIF: { const float q = 1.0f - rf; v = lf < q ? lf : q; wl = lf == v ? 1.0f : 0.0f; wr = (1.0f - rf) == v ? 1.0f : 0.0f; } break;
    case PSGPU_OP_SMOOTHDIF: v = lf * (1.0f - rf); wl = lf == v ? 1.0f : 0.0f; wr = (1.0f - rf) == v ? 1.0f : 0.0f; break;
    default: weighted = false; break;
    }
    for (int k = 0; k < 3; ++k) {
        if (weighted) D.zeroCol[op][k] = wl * cl[k] + wr * cr[k];
        else if (t >= PSGPU_OP_WARPTWIST && t <= PSGPU_OP_WARPSHEAR) D.zeroCol[op][k] = cl[k];
        else D.zeroCol[op][k] = 0.0f;  // not used: zero subtrees contain only the types above
    }
}

inline int build_device_model(const PsSoaBlobPrims& P, const PsSoaPrimMatrices& Mx, const PsSoaBlobOps& O, DevModel& D) {
    memset(&D, 0, sizeof(D));
    if (P.ctPrims == 0 || P.ctPrims > 128 || O.ctOps > 128) return PSGPU_RET_PARAM_ERROR;
    D.ctPrims = P.ctPrims;
    D.ctOps = O.ctOps;
    if (O.ctOps == 0) {
        for (uint32_t i = 0; i < P.ctPrims; ++i) {
            Instr s{};
            s.kind = kSumPrim;
            s.idx = (uint16_t)i;
            D.instr[i] = s;
        }
        D.nInstr = P.ctPrims;
        D.nSlots = 1;
    } else {
        ProgramBuilder b(O);
        b.emit(0, 0, 0);
        if (!b.ok) return PSGPU_RET_INVALID_BVH;
        D.nInstr = (uint32_t)b.prog.size();
        std::copy(b.prog.begin(), b.prog.end(), D.instr);
        D.nSlots = (uint32_t)std::max(1, b.maxSlot);
    }
    for (uint32_t i = 0; i < 128; ++i) {
        DevOp& d = D.ops[i];
        d.lo[0] = O.vBoxLoX[i]; d.lo[1] = O.vBoxLoY[i]; d.lo[2] = O.vBoxLoZ[i];
        d.hi[0] = O.vBoxHiX[i]; d.hi[1] = O.vBoxHiY[i]; d.hi[2] = O.vBoxHiZ[i];
        d.resY = O.resY[i];
        d.type = O.opType[i];
    }
    // the zero-subtree colours (zero_col above); unreachable ops keep zero
    const float* const pc[3] = {P.colorX, P.colorY, P.colorZ};
    if (O.ctOps > 0) zero_col(O, pc, D, 0);
    // every one of the 128 prim slots is uploaded: the reference evaluates whatever
    // index an op names, even past ctPrims (SOABlobPrims keeps all 128 entries)
    for (uint32_t i = 0; i < 128; ++i) {
        DevPrim& d = D.prims[i];
        d.pos[0] = P.posX[i]; d.pos[1] = P.posY[i]; d.pos[2] = P.posZ[i];
        d.dir[0] = P.dirX[i]; d.dir[1] = P.dirY[i]; d.dir[2] = P.dirZ[i];
        d.res[0] = P.resX[i]; d.res[1] = P.resY[i]; d.res[2] = P.resZ[i];
        d.col[0] = P.colorX[i]; d.col[1] = P.colorY[i]; d.col[2] = P.colorZ[i];
        d.type = P.skeletType[i];
        const uint32_t im = P.idxMatrix[i];
        d.hasMatrix = im != 0;
        if (im != 0) {
            if (im >= 128) return PSGPU_RET_PARAM_ERROR;
            memcpy(d.mat, &Mx.matrix[im * PSGPU_PRIM_MATRIX_STRIDE], 12 * sizeof(float));
        }
        // exact-culling eligibility (see make_cull_mask in psgpu_kernels.hip)
        bool c = !d.hasMatrix && finite3(d.pos);
        switch (d.type) {
        case PSGPU_PRIM_POINT: break;
        case PSGPU_PRIM_LINE: {
            const double ux = (double)d.dir[0] - d.pos[0], uy = (double)d.dir[1] - d.pos[1],
                         uz = (double)d.dir[2] - d.pos[2];
            c = c && finite3(d.dir) && (ux * ux + uy * uy + uz * uz) > 1e-6;
        } break;
        case PSGPU_PRIM_CUBE: c = c && std::isfinite(d.res[0]) && d.res[0] >= 0.0f; break;
        case PSGPU_PRIM_CYLINDER: {
            const double n2 = (double)d.dir[0] * d.dir[0] + (double)d.dir[1] * d.dir[1] + (double)d.dir[2] * d.dir[2];
            c = c && finite3(d.dir) && std::fabs(n2 - 1.0) < 1e-4 && d.res[0] >= 0.0f && d.res[1] >= 0.0f &&
                std::isfinite(d.res[0]) && std::isfinite(d.res[1]);
        } break;
        default: c = false; break;
        }
        // culling skeleton (CullSeg, psgpu_model.h): a lower bound of the distance
        CullSeg& cs = D.cull[i];
        memset(&cs, 0, sizeof(cs));
        const float inf = std::numeric_limits<float>::infinity();
        cs.radius = inf;  // never culled unless eligible below
        cs.tmin = 0.0f;
        cs.tmax = 1.0f;
        cs.axisClear = -inf;
        cs.boxHalf = inf;  // not an axis-aligned box: no gap form
        uint32_t flags = c ? 1u : 0u;
        if (c) {
            for (int a = 0; a < 3; ++a) cs.a[a] = d.pos[a];
            cs.radius = 0.0f;
            double uu = 0.0;
            if (d.type == PSGPU_PRIM_LINE) {
                for (int a = 0; a < 3; ++a) cs.u[a] = d.dir[a] - d.pos[a];
                cs.tmin = -inf;
                cs.tmax = inf;
                flags |= 2u;
            } else if (d.type == PSGPU_PRIM_CYLINDER) {
                for (int a = 0; a < 3; ++a) cs.u[a] = d.res[1] * d.dir[a];  // axis segment, length h
                cs.radius = d.res[0];
                cs.axisClear = 0.05f;
                flags |= 4u;
            } else if (d.type == PSGPU_PRIM_CUBE) {
                cs.radius = (float)(d.res[0] * 1.7320508075688772 * (1.0 + 1e-6));
                cs.boxHalf = d.res[0];
            } else {
                cs.boxHalf = 0.0f;  // Point
            }
            for (int a = 0; a < 3; ++a) uu += (double)cs.u[a] * cs.u[a];
            cs.invUU = uu > 0.0 ? (float)(1.0 / uu) : 0.0f;
            if (d.type == PSGPU_PRIM_CYLINDER && uu == 0.0) {  // h = 0: no axis direction
                flags &= ~1u;
                cs.radius = inf;
            }
        } else if (d.type == PSGPU_PRIM_TRIANGLE) {
            cs.radius = -inf;  // field exactly 0 everywhere (dist2 = FLT_MAX)
        }
        if (i >= P.ctPrims) {  // (the culling masks only cover ctPrims)
            cs.radius = inf;
            cs.boxHalf = inf;
        }
        d.cullable = flags;
    }
    // field bounds (k_precheck, prim_bound in psgpu_device.h) need every primitive the
    // walk evaluates to have a true-distance bound with sane parameters (the culling
    // eligibility above) or be a Triangle (field 0), and every op a monotone map
    bool bnd = D.nInstr > 0;
    for (uint32_t k = 0; k < D.nInstr; ++k) {
        const Instr& I = D.instr[k];
        if (I.kind == kOp && !((I.type >= 14 && I.type <= 18) || (I.type >= 22 && I.type <= 25))) bnd = false;
        if (I.kind == kPrim || I.kind == kSumPrim) {
            const DevPrim& q = D.prims[I.idx];
            if (!(q.type == PSGPU_PRIM_TRIANGLE || (q.cullable & 1u))) bnd = false;
        }
    }
    D.boundable = bnd ? 1u : 0u;
    // the primitives that, all culled over a box, leave the root exactly +0 there (k_sieve)
    D.rootZeroValid = root_zero_set(D, D.rootZero) ? 1u : 0u;
    if (!D.rootZeroValid) D.rootZero[0] = D.rootZero[1] = 0ull;
    return PSGPU_RET_SUCCESS;
}

inline void lattice_dims(float cs, const PsVec3f& lo, const PsVec3f& hi, uint32_t d[3]) {
    const float ext[3] = {hi.x - lo.x, hi.y - lo.y, hi.z - lo.z};
    for (int a = 0; a < 3; ++a) {
        const float q = ext[a] / cs;
        const int cells = (int)std::ceil(q);
        int n = cells / PSGPU_CELLS_PER_MPU;
        if (cells % PSGPU_CELLS_PER_MPU != 0) ++n;
        d[a] = n > 0 ? (uint32_t)n : 0u;
    }
}

inline int translate_blobtree_type(int t) {
    // _constSettings.h:26-38 -> PS_Polygonizer.h:84-91
    static const int map[29] = {
        PSGPU_PRIM_POINT, PSGPU_PRIM_LINE, PSGPU_PRIM_CYLINDER, PSGPU_PRIM_DISC, PSGPU_PRIM_RING,
        PSGPU_PRIM_POLYGON, PSGPU_PRIM_CUBE, PSGPU_PRIM_TRIANGLE, PSGPU_PRIM_CATMULLROM, PSGPU_PRIM_SKELETON,
        PSGPU_PRIM_QUADRICPOINT, PSGPU_PRIM_HALFPLANE, PSGPU_PRIM_NULL, -1 /* Instance */,
        PSGPU_OP_UNION, PSGPU_OP_INTERSECT, PSGPU_OP_DIF, PSGPU_OP_SMOOTHDIF, PSGPU_OP_BLEND,
        PSGPU_OP_RICCIBLEND, PSGPU_OP_GRADIENTBLEND, PSGPU_PRIM_FASTQPS, PSGPU_OP_PCM, PSGPU_OP_CACHE,
        PSGPU_OP_WARPTWIST, PSGPU_OP_WARPTAPER, PSGPU_OP_WARPBEND, PSGPU_OP_WARPSHEAR, PSGPU_OP_TEXTURE};
    return (t >= 0 && t < 29) ? map[t] : -1;
}

// PrepareBBoxes (PS_Polygonizer.cpp:55-309) with iso distance ISO_DIST + 5*MIN_CELL_SIZE.
inline int prepare_bboxes(PsSoaBlobPrims* P, PsSoaBoxMatrices* BM, PsSoaBlobOps* O) {
    if (!P || !O || P->ctPrims == 0 || P->ctPrims > 128) return PSGPU_RET_PARAM_ERROR;
    const float iso = PSGPU_ISO_DIST + 5.0f * PSGPU_MIN_CELL_SIZE;
    float* boxLo[3] = {P->vPrimBoxLoX, P->vPrimBoxLoY, P->vPrimBoxLoZ};
    float* boxHi[3] = {P->vPrimBoxHiX, P->vPrimBoxHiY, P->vPrimBoxHiZ};
    for (uint32_t i = 0; i < P->ctPrims; ++i) {
        const float p[3] = {P->posX[i], P->posY[i], P->posZ[i]};
        const float d[3] = {P->dirX[i], P->dirY[i], P->dirZ[i]};
        float lo[3], hi[3];
        for (int a = 0; a < 3; ++a) { lo[a] = boxLo[a][i]; hi[a] = boxHi[a][i]; }
        switch (P->skeletType[i]) {
        case PSGPU_PRIM_POINT:
            for (int a = 0; a < 3; ++a) { lo[a] = p[a] - iso; hi[a] = p[a] + iso; }
            break;
        case PSGPU_PRIM_LINE:
            for (int a = 0; a < 3; ++a) {
                const float e = iso * 1.0f + (3.0f * iso) * (d[a] - p[a]);
                lo[a] = p[a] - e; hi[a] = d[a] + e;
            }
            break;
        case PSGPU_PRIM_RING: case PSGPU_PRIM_DISC: {
            const float r = P->resX[i] + iso;
            for (int a = 0; a < 3; ++a) {
                const float e = (r + iso) * (1.0f - d[a]) + iso * d[a];
                lo[a] = p[a] - e; hi[a] = p[a] + e;
            }
        } break;
        case PSGPU_PRIM_CYLINDER: {
            const float r = P->resX[i], h = P->resY[i];
            for (int a = 0; a < 3; ++a) {
                const float s1 = p[a] + h * d[a];
                const float e = (iso + r) * 1.0f + (0.5f * iso) * d[a];
                lo[a] = p[a] - e; hi[a] = s1 + e;
            }
        } break;
        case PSGPU_PRIM_CUBE: {
            const float s = P->resX[i] + iso;
            for (int a = 0; a < 3; ++a) { lo[a] = p[a] - s; hi[a] = p[a] + s; }
        } break;
        case PSGPU_PRIM_TRIANGLE: {
            const float r[3] = {P->resX[i], P->resY[i], P->resZ[i]};
            for (int a = 0; a < 3; ++a) {
                float mn = p[a] < d[a] ? p[a] : d[a];
                mn = mn < r[a] ? mn : r[a];
                float mx = p[a] > d[a] ? p[a] : d[a];
                mx = mx > r[a] ? mx : r[a];
                lo[a] = mn - iso; hi[a] = mx + iso;
            }
        } break;
        default: break;
        }
        const uint32_t im = P->idxMatrix[i];
        if (im != 0 && BM && im < BM->count) {  // mat4Transform, PS_MATRIX4.h:199-209 (column vectors)
            const float* M = &BM->matrix[im * PSGPU_BOX_MATRIX_STRIDE];
            float tl[3], th[3];
            for (int r = 0; r < 3; ++r) {
                tl[r] = ((M[r] * lo[0] + M[4 + r] * lo[1]) + M[8 + r] * lo[2]) + M[12 + r];
                th[r] = ((M[r] * hi[0] + M[4 + r] * hi[1]) + M[8 + r] * hi[2]) + M[12 + r];
            }
            memcpy(lo, tl, sizeof(lo));
            memcpy(hi, th, sizeof(hi));
        }
        for (int a = 0; a < 3; ++a) { boxLo[a][i] = lo[a]; boxHi[a][i] = hi[a]; }
        float* bl = &P->bboxLo.x;
        float* bh = &P->bboxHi.x;
        for (int a = 0; a < 3; ++a) {
            if (i == 0) { bl[a] = lo[a]; bh[a] = hi[a]; }
            else { bl[a] = bl[a] < lo[a] ? bl[a] : lo[a]; bh[a] = bh[a] > hi[a] ? bh[a] : hi[a]; }
        }
    }
    if (O->ctOps > 0) {  // op boxes bottom-up (:238-307) as a post-order walk
        std::vector<uint8_t> done(256, 0);
        std::vector<uint32_t> st{0};
        size_t guard = 0;
        while (!st.empty()) {
            if (++guard > 100000) return PSGPU_RET_INVALID_BVH;
            const uint32_t op = st.back();
            if (op >= 128) return PSGPU_RET_INVALID_BVH;
            const uint32_t L = O->opLeftChild[op], R = O->opRightChild[op];
            const int lop = (O->opChildKind[op] & 2) >> 1, rop = O->opChildKind[op] & 1;
            if ((lop && !done[L]) || (rop && !done[R])) {
                if (lop && !done[L]) st.push_back(L);
                if (rop && !done[R]) st.push_back(R);
                continue;
            }
            st.pop_back();
            // a primitive child id is not checked against 128 here (the reference reads whatever
            // the tree names): ids up to 198 stay inside PsSoaBlobPrims, 199-255 read vPrimBoxHi*
            // past the end of the struct (an open finding).  build_device_model rejects
            // such a tree wherever the walk would evaluate that child
            auto get =[&](int isOp, uint32_t k, float lo[3], float hi[3]) {
                if (isOp) {
                    lo[0] = O->vBoxLoX[k]; lo[1] = O->vBoxLoY[k]; lo[2] = O->vBoxLoZ[k];
                    hi[0] = O->vBoxHiX[k]; hi[1] = O->vBoxHiY[k]; hi[2] = O->vBoxHiZ[k];
                } else {
                    for (int a = 0; a < 3; ++a) { lo[a] = boxLo[a][k]; hi[a] = boxHi[a][k]; }
                }
            };
            float l0[3], h0[3], l1[3], h1[3];
            get(lop, L, l0, h0);
            get(rop, R, l1, h1);
            float* oLo[3] = {O->vBoxLoX, O->vBoxLoY, O->vBoxLoZ};
            float* oHi[3] = {O->vBoxHiX, O->vBoxHiY, O->vBoxHiZ};
            for (int a = 0; a < 3; ++a) {
                oLo[a][op] = l0[a] < l1[a] ? l0[a] : l1[a];
                oHi[a][op] = h0[a] > h1[a] ? h0[a] : h1[a];
            }
            done[op] = 1;
        }
    }
    return PSGPU_RET_SUCCESS;
}

// Contiguous ranges of near-equal cost: bounds[k] = begin + the first index whose cost
// prefix reaches k/parts of the total (bounds[0] = begin, bounds[parts] = begin + n).
inline int split_costs(const uint32_t* costs, uint32_t n, uint32_t parts, uint32_t begin, uint32_t* bounds) {
    if (!bounds || parts == 0 || (n && !costs)) return PSGPU_RET_PARAM_ERROR;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += costs[i];
    bounds[0] = begin;
    uint64_t acc = 0;
    uint32_t i = 0;
    for (uint32_t k = 1; k < parts; ++k) {
        const uint64_t target = (total * k + parts / 2) / parts;
        while (i < n && acc + costs[i] / 2 < target) acc += costs[i++];
        bounds[k] = begin + i;
    }
    bounds[parts] = begin + n;
    return PSGPU_RET_SUCCESS;
}

}  // namespace psgpu
