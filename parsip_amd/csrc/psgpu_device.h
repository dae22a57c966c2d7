// psgpu_device.h — device code shared by the static kernels (psgpu_kernels.hip) and the
// run-time specialised kernels (psgpu_jit.cpp, compiled with hiprtc).  Must compile
// under hiprtc: no system headers.
//
// Reference semantics restated here (Parsip100/PS_SimdPoly/include/):
//   computePrimitiveField           PS_Polygonizer.cpp:934-1179
//   ComputeWyvillFieldValueSquare_  PS_Polygonizer.h:397-407
//   FieldComputer::fieldValue       PS_Polygonizer.cpp:1184-1376 (op-box pruning :1228-1252)
//   FieldComputer::fieldValueAndColor :1378-1551, normal :1598-1622
//   CMPUProcessor::process_cells_simd :475-829
// Every fp32 expression keeps the reference's operation order; builds use
// -ffp-contract=off, IEEE division/sqrt (sqrtf, '/') and IEEE denormals.  max/min are the
// SSE definitions (a>b?a:b, a<b?a:b; PS_SIMDVecN.h:388-389), masks are {0,1} multipliers.
#pragma once
#include "psgpu_model.h"

namespace psgpu {

// ---------------------------------------------------------------------------
// The model is read through the constant address space so that every wave-uniform
// access (walk program, op boxes, primitive parameters) is an s_load into SGPRs.
typedef const __attribute__((address_space(4))) DevModel* ModelPtr;
typedef const __attribute__((address_space(4))) DevPrim CPrim;
typedef const __attribute__((address_space(4))) DevOp COp;
typedef const __attribute__((address_space(4))) CubeTablesDev* TablePtr;
__device__ __forceinline__ ModelPtr as_const(const DevModel* m) { return (ModelPtr)m; }
__device__ __forceinline__ TablePtr as_const(const CubeTablesDev* t) { return (TablePtr)t; }

__device__ __forceinline__ Instr load_instr(ModelPtr M, int pc) {
    typedef const __attribute__((address_space(4))) uint32_t* CU32;
    const CU32 w = (CU32)(&M->instr[pc]);
    const uint32_t words[3] = {w[0], w[1], w[2]};
    Instr I;
    __builtin_memcpy(&I, words, 12);
    return I;
}

__device__ __forceinline__ float max_ref(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float min_ref(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float m01(bool c) { return c ? 1.0f : 0.0f; }
__device__ __forceinline__ int lane_id() { return __lane_id(); }
__device__ __forceinline__ uint64_t ballot(bool v) { return __ballot(v); }

// 1 if any lane of this lane's 4-lane group has v set (the reference's 4-wide SIMD
// group: VecNMask(inside) == PS_SIMD_ALLZERO, PS_Polygonizer.cpp:1243).
// DPP quad_perm swaps within each 4-lane group: [1,0,3,2] then [2,3,0,1].
__device__ __forceinline__ bool quad_any(bool v) {
    int x = v ? 1 : 0;
    x |= __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, false);
    x |= __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, false);
    return x != 0;
}

template <int GROUP>
__device__ __forceinline__ bool group_any(bool v) {
    if (GROUP == 4) return quad_any(v);
    return v;
}

// Cross-lane work on DPP (no LDS crossbar round trips): quad_perm [1,0,3,2] = 0xB1,
// [2,3,0,1] = 0x4E, row_half_mirror = 0x141, row_mirror = 0x140, row_shr:n = 0x110 + n,
// row_bcast:15 = 0x142, row_bcast:31 = 0x143.
#define PSGPU_DPP_F(v, ctrl) __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), (ctrl), 0xF, 0xF, false))

// Value of lane S of this lane's quad.
template <int S>
__device__ __forceinline__ float quad_bcast(float v) { return PSGPU_DPP_F(v, S * 0x55); }

// Wave-uniform min / max (NaNs must be excluded by the caller).
__device__ __forceinline__ float wave_min(float v) {
    v = fminf(v, PSGPU_DPP_F(v, 0xB1));
    v = fminf(v, PSGPU_DPP_F(v, 0x4E));
    v = fminf(v, PSGPU_DPP_F(v, 0x141));
    v = fminf(v, PSGPU_DPP_F(v, 0x140));
    return fminf(fminf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)),
                       __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16))),
                 fminf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)),
                       __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48))));
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, PSGPU_DPP_F(v, 0xB1));
    v = fmaxf(v, PSGPU_DPP_F(v, 0x4E));
    v = fmaxf(v, PSGPU_DPP_F(v, 0x141));
    v = fmaxf(v, PSGPU_DPP_F(v, 0x140));
    return fmaxf(fmaxf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)),
                       __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16))),
                 fmaxf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)),
                       __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48))));
}
// Inclusive prefix sum over the wave (Hillis-Steele in 16-lane rows, then row broadcasts).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);
    return v;
}
// PSGPU_FOR_N(stmt): stmt once for each point n < N (N <= 8, a template parameter in
// scope), unrolled by the preprocessor and `if constexpr` instead of a loop (the
// generated tree walks emit thousands of these; see psgpu_jit.cpp, Gen::FN).
#define PSGPU_N_AT(k, ...)                 \
    if constexpr (N > k) {                 \
        constexpr int n = k;               \
        __VA_ARGS__                        \
    }
#define PSGPU_FOR_N(...)                                                                              \
    {                                                                                                 \
        static_assert(N >= 1 && N <= 8, "PSGPU_FOR_N: 1..8 points per lane");                         \
        PSGPU_N_AT(0, __VA_ARGS__) PSGPU_N_AT(1, __VA_ARGS__) PSGPU_N_AT(2, __VA_ARGS__)              \
        PSGPU_N_AT(3, __VA_ARGS__) PSGPU_N_AT(4, __VA_ARGS__) PSGPU_N_AT(5, __VA_ARGS__)              \
        PSGPU_N_AT(6, __VA_ARGS__) PSGPU_N_AT(7, __VA_ARGS__)                                         \
    }

// Value of a wave-uniform lane (scalar read).
__device__ __forceinline__ uint32_t lane_value(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}
// A value the wave holds in every lane, as a scalar (SGPR): branches on it are scalar, and
// the compiler sees the uniformity its divergence analysis cannot prove (e.g. anything
// derived from threadIdx.x >> 6).
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int wave_index() { return (int)(threadIdx.x >> 6); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return (uint64_t)uniform((uint32_t)v) | ((uint64_t)uniform((uint32_t)(v >> 32)) << 32);
}

// ---------------------------------------------------------------------------
// Primitive fields.  dist2 per skeleton type, then Wyvill.
// PR: a DevPrim in the constant address space (parameters loaded at run time) or a
// constexpr BakedPrim (parameters compiled into the code, psgpu_jit.cpp mode 2).
struct BakedPrim {
    float pos[3], dir[3], res[3], col[3], mat[12];
};
struct BakedOp {
    float lo[3], hi[3], resY;
};

// Parameter groups of the generated walk (psgpu_jit.cpp, mode 1): the parameters a subtree's
// walk reads, loaded into SGPRs together at the subtree's entry, so the wave waits for its
// scalar loads once per group instead of once per primitive (every wait is lgkmcnt(0):
// scalar loads return out of order).  The empty asm statements pin each value in an SGPR
// there, so the loads are not sunk back to their first use.
template <int TYPE>
__device__ __forceinline__ constexpr bool prim_uses_dir() {
    return TYPE == PSGPU_T_LINE || TYPE == PSGPU_T_CYLINDER || TYPE == PSGPU_T_DISC || TYPE == PSGPU_T_RING;
}
template <int TYPE>
__device__ __forceinline__ constexpr int prim_res_count() {
    return TYPE == PSGPU_T_CYLINDER ? 2 : ((TYPE == PSGPU_T_CUBE || TYPE == PSGPU_T_DISC || TYPE == PSGPU_T_RING) ? 1 : 0);
}
template <int TYPE>
__device__ __forceinline__ constexpr bool prim_uses_pos() {
    return TYPE == PSGPU_T_POINT || TYPE == PSGPU_T_LINE || TYPE == PSGPU_T_CYLINDER || TYPE == PSGPU_T_CUBE ||
           TYPE == PSGPU_T_DISC || TYPE == PSGPU_T_RING;
}
#define PSGPU_PIN(v) asm volatile("" ::"s"(v))
template <int TYPE, bool MAT>
__device__ __forceinline__ void load_prim(CPrim& S, BakedPrim& r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (prim_uses_pos<TYPE>()) r.pos[k] = S.pos[k];
        if (prim_uses_dir<TYPE>()) r.dir[k] = S.dir[k];
        if (k < prim_res_count<TYPE>()) r.res[k] = S.res[k];
    }
    if (MAT) {
#pragma unroll
        for (int k = 0; k < 12; ++k) r.mat[k] = S.mat[k];
    }
}
template <int TYPE, bool MAT>
__device__ __forceinline__ void pin_prim(const BakedPrim& r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (prim_uses_pos<TYPE>()) PSGPU_PIN(r.pos[k]);
        if (prim_uses_dir<TYPE>()) PSGPU_PIN(r.dir[k]);
        if (k < prim_res_count<TYPE>()) PSGPU_PIN(r.res[k]);
    }
    if (MAT) {
#pragma unroll
        for (int k = 0; k < 12; ++k) PSGPU_PIN(r.mat[k]);
    }
}
template <class OP>
__device__ __forceinline__ void load_op(OP& S, BakedOp& r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.lo[k] = S.lo[k];
        r.hi[k] = S.hi[k];
    }
}
__device__ __forceinline__ void pin_op(const BakedOp& r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        PSGPU_PIN(r.lo[k]);
        PSGPU_PIN(r.hi[k]);
    }
}

template <int TYPE, class PR>
__device__ __forceinline__ float prim_dist2(PR& P, float x, float y, float z) {
    float d2 = 0.0f;
    if (TYPE == PSGPU_T_POINT) {  // :975-983
        float dx = P.pos[0] - x, dy = P.pos[1] - y, dz = P.pos[2] - z;
        d2 = (dx * dx + dy * dy) + dz * dz;
    } else if (TYPE == PSGPU_T_LINE) {  // :984-1011 (pos = start, dir = end), not clamped
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
    } else if (TYPE == PSGPU_T_CYLINDER) {  // :1012-1039 (axis dir, r = resX, h = resY)
        float px = x - P.pos[0], py = y - P.pos[1], pz = z - P.pos[2];
        float yy = (px * P.dir[0] + py * P.dir[1]) + pz * P.dir[2];
        float rr = ((px * px + py * py) + pz * pz) - yy * yy;
        float xx = max_ref(0.0f, sqrtf(rr) - P.res[0]);
        float mask = m01(yy > 0.0f);
        yy = mask * max_ref(0.0f, yy - P.res[1]) + (1.0f - mask) * yy;
        d2 = xx * xx + yy * yy;
    } else if (TYPE == PSGPU_T_TRIANGLE) {  // :1040-1057 distance stub
        d2 = 3.402823466e+38f;
    } else if (TYPE == PSGPU_T_CUBE) {  // :1059-1097 (half side resX)
        float side = P.res[0], mside = -1.0f * P.res[0];
        float dif[3] = {x - P.pos[0], y - P.pos[1], z - P.pos[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            float mm = m01(mside > dif[a]);
            float mp = m01(dif[a] > side);
            float dl = (dif[a] + side) * mm + (dif[a] - side) * mp;
            d2 = (a == 0) ? dl * dl : d2 + dl * dl;
        }
    } else if (TYPE == PSGPU_T_DISC) {  // :1099-1132
        float dX = x - P.pos[0], dY = y - P.pos[1], dZ = z - P.pos[2];
        float nX = P.dir[0], nY = P.dir[1], nZ = P.dir[2], r = P.res[0];
        float dot = (nX * dX + nY * dY) + nZ * dZ;
        float rX = dX - nX * dot, rY = dY - nY * dot, rZ = dZ - nZ * dot;
        dot = (rX * rX + rY * rY) + rZ * rZ;
        float rs = 1.0f / sqrtf(dot);  // _mm_rsqrt_ps in the reference (vendor specific)
        rX = rX * rs; rY = rY * rs; rZ = rZ * rs;
        nX = r * rX - dX; nY = r * rY - dY; nZ = r * rZ - dZ;
        float mask = m01(r * r >= dot);
        d2 = mask * (((dX * dX + dY * dY) + dZ * dZ) - dot) + (1.0f - mask) * ((nX * nX + nY * nY) + nZ * nZ);
    } else if (TYPE == PSGPU_T_RING) {  // :1134-1173
        float dX = x - P.pos[0], dY = y - P.pos[1], dZ = z - P.pos[2];
        float nX = P.dir[0], nY = P.dir[1], nZ = P.dir[2], r = P.res[0];
        float dot = (nX * dX + nY * dY) + nZ * dZ;
        float rX = dX - nX * dot, rY = dY - nY * dot, rZ = dZ - nZ * dot;
        dot = (rX * rX + rY * rY) + rZ * rZ;
        float mask = m01(dot == 0.0f);
        dot = 1.0f / sqrtf(dot);
        rX = rX * dot; rY = rY * dot; rZ = rZ * dot;
        nX = r * rX - dX; nY = r * rY - dY; nZ = r * rZ - dZ;
        d2 = mask * (((r * r + dX * dX) + dY * dY) + dZ * dZ) + (1.0f - mask) * ((nX * nX + nY * nY) + nZ * nZ);
    }
    // any other code: no case in the reference switch, dist2 stays 0 (field 1)
    return d2;
}

__device__ __forceinline__ float wyvill(float d2) {
    float t = 1.0f - d2;
    float f = (t * t) * t;
    return max_ref(0.0f, f);
}

template <int TYPE, bool MAT, class PR>
__device__ __forceinline__ float prim_field_t(PR& P, float pX, float pY, float pZ) {
    float x = pX, y = pY, z = pZ;
    if (MAT) {  // :948-970, rows ((m0*x + m1*y) + m2*z) + m3
        x = ((P.mat[0] * pX + P.mat[1] * pY) + P.mat[2] * pZ) + P.mat[3];
        y = ((P.mat[4] * pX + P.mat[5] * pY) + P.mat[6] * pZ) + P.mat[7];
        z = ((P.mat[8] * pX + P.mat[9] * pY) + P.mat[10] * pZ) + P.mat[11];
    }
    return wyvill(prim_dist2<TYPE, PR>(P, x, y, z));
}

// run-time dispatch (interpreter)
__device__ __forceinline__ float prim_field(CPrim& P, float pX, float pY, float pZ) {
    float x = pX, y = pY, z = pZ;
    if (P.hasMatrix) {
        x = ((P.mat[0] * pX + P.mat[1] * pY) + P.mat[2] * pZ) + P.mat[3];
        y = ((P.mat[4] * pX + P.mat[5] * pY) + P.mat[6] * pZ) + P.mat[7];
        z = ((P.mat[8] * pX + P.mat[9] * pY) + P.mat[10] * pZ) + P.mat[11];
    }
    float d2;
    switch (P.type) {
    case PSGPU_T_POINT: d2 = prim_dist2<PSGPU_T_POINT, CPrim>(P, x, y, z); break;
    case PSGPU_T_LINE: d2 = prim_dist2<PSGPU_T_LINE, CPrim>(P, x, y, z); break;
    case PSGPU_T_CYLINDER: d2 = prim_dist2<PSGPU_T_CYLINDER, CPrim>(P, x, y, z); break;
    case PSGPU_T_TRIANGLE: d2 = prim_dist2<PSGPU_T_TRIANGLE, CPrim>(P, x, y, z); break;
    case PSGPU_T_CUBE: d2 = prim_dist2<PSGPU_T_CUBE, CPrim>(P, x, y, z); break;
    case PSGPU_T_DISC: d2 = prim_dist2<PSGPU_T_DISC, CPrim>(P, x, y, z); break;
    case PSGPU_T_RING: d2 = prim_dist2<PSGPU_T_RING, CPrim>(P, x, y, z); break;
    default: d2 = 0.0f; break;
    }
    return wyvill(d2);
}

// Binary op field (:1282-1338); `last` is the previous op's field (stale outField).
__device__ __forceinline__ float op_field(uint32_t type, float lf, float rf, float resY, float last) {
    switch (type) {
    case PSGPU_T_BLEND: return lf + rf;
    case PSGPU_T_RICCI: {  // fast_pow, PS_SIMDVecN.h:122-128 (rcp -> IEEE 1/x)
        const float base = lf + rf;
        float den = resY * base;
        den = resY - den;
        den = base + den;
        return base * (1.0f / den);
    }
    case PSGPU_T_UNION: return max_ref(lf, rf);
    case PSGPU_T_INTERSECT: return min_ref(lf, rf);
    case PSGPU_T_DIF: return min_ref(lf, 1.0f - rf);
    case PSGPU_T_SMOOTHDIF: return lf * (1.0f - rf);
    case 22: case 23: case 24: case 25: return lf;  // warps: identity
    default: return last;
    }
}

// Op colour weights (:1472-1522); returns false when the op keeps a colour instead.
__device__ __forceinline__ bool op_colour_weights(uint32_t type, float lf, float rf, float v, float* wl, float* wr) {
    switch (type) {
    case PSGPU_T_BLEND: case PSGPU_T_RICCI:
        *wl = 2.0f * (0.5f + lf) - 1.0f;
        *wr = 2.0f * (0.5f + rf) - 1.0f;
        return true;
    case PSGPU_T_UNION: case PSGPU_T_INTERSECT:
        *wl = m01((v - lf) == 0.0f);
        *wr = m01((v - rf) == 0.0f);
        return true;
    case PSGPU_T_DIF: case PSGPU_T_SMOOTHDIF:
        *wl = m01(lf == v);
        *wr = m01((1.0f - rf) == v);
        return true;
    default:
        return false;
    }
}

// ---------------------------------------------------------------------------
// Exact culling (never changes a bit of output).  A primitive whose support cannot
// reach any point of the wave has computed dist2 >= 1, i.e. field exactly +0, and
// is not evaluated.  Every cullable primitive has a skeleton segment (CullSeg) whose
// distance minus a radius bounds its distance from below and is 1-Lipschitz: Point
// (a point), infinite Line (an unbounded segment), capped Cylinder with |axis| = 1
// (its axis segment, radius r), axis-aligned Cube (its centre, radius s*sqrt(3); and
// the cube itself, as a box).  For the wave's AABB with centre c and half-diagonal h every
// point q then has d(q) >= d(c) - h, and the tighter bounds that treat the AABB as a box
// and not as its sphere (cull_one, psgpu_model.h).  The host marks a prim cullable only without a matrix and with
// finite, well-conditioned parameters; Cylinder also needs the AABB clear of its
// infinite axis (where the reference's sqrt of a rounded-negative value is NaN).  The
// margin d^2 >= 1.02 covers fp32 rounding of the reference formulas by orders of
// magnitude.  Triangle is a constant +0 (dist2 = FLT_MAX) and is always culled.
// inLo / inHi: the op-inside mask that rides with it (op_inside_box, psgpu_model.h): bit k set
// means every point of the wave lies inside op k's box along one axis, so op k's pruning test
// cannot prune and the generated walks skip it.  Made per queued MPU by k_precheck only; every
// other source of a CullMask (the wave's own box: S1, k_finish's off-segment fallback, the
// probe) leaves it 0, where every test runs.
struct CullMask {
    uint64_t lo, hi;
    uint64_t inLo, inHi;
};
__device__ __forceinline__ bool op_inside(const CullMask& cm, uint32_t k) {
    return k < 64 ? ((cm.inLo >> k) & 1ull) : ((cm.inHi >> (k - 64)) & 1ull);
}

// This lane's culling segments (prims `lane` and 64 + `lane`), loaded once and early: the
// loads do not depend on the box, so they overlap the rest of a kernel's prologue.
struct CullLanes {
    CullSeg s[2];
    bool two;  // ctPrims > 64
};

__device__ __forceinline__ CullSeg load_cullseg(ModelPtr M, int i) {
    typedef const __attribute__((address_space(4))) float* CF;
    const CF f = (CF)(&M->cull[i]);  // 12 consecutive floats: the compiler emits 16-B loads
    CullSeg S;
    S.a[0] = f[0]; S.a[1] = f[1]; S.a[2] = f[2];
    S.u[0] = f[3]; S.u[1] = f[4]; S.u[2] = f[5];
    S.invUU = f[6]; S.radius = f[7];
    S.tmin = f[8]; S.tmax = f[9]; S.axisClear = f[10]; S.boxHalf = f[11];
    return S;
}

__device__ __forceinline__ CullLanes load_cull_lanes(ModelPtr M) {
    CullLanes L;
    L.two = M->ctPrims > 64u;
    L.s[0] = load_cullseg(M, lane_id());
    if (L.two) L.s[1] = load_cullseg(M, 64 + lane_id());
    return L;
}

// cull_one / cull_box: psgpu_model.h (host and device)
__device__ __forceinline__ CullMask cull_mask_from(const CullLanes& L, float x0, float y0, float z0, float x1,
                                                   float y1, float z1) {
    CullMask cm{0ull, 0ull};
    float c[3], h, he[3];
    if (!cull_box(x0, y0, z0, x1, y1, z1, c, &h, he)) return cm;
    cm.lo = ballot(cull_one(L.s[0], c[0], c[1], c[2], h, he));
    if (L.two) cm.hi = ballot(cull_one(L.s[1], c[0], c[1], c[2], h, he));
    return cm;
}

__device__ __forceinline__ CullMask cull_mask_box(ModelPtr M, float x0, float y0, float z0, float x1, float y1,
                                                  float z1) {
    return cull_mask_from(load_cull_lanes(M), x0, y0, z0, x1, y1, z1);
}

// Cull mask for the AABB of this wave's points (all 64 lanes must participate),
// optionally grown by `ext` on the high side of every axis.
__device__ __forceinline__ CullMask cull_mask_points(const CullLanes& L, float px, float py, float pz, bool enable,
                                                     float ext = 0.0f) {
    if (!enable) return CullMask{0ull, 0ull};
    // a NaN coordinate (fminf/fmaxf would hide it) disables culling for the wave
    if (ballot(!(px == px) || !(py == py) || !(pz == pz)) != 0ull) return CullMask{0ull, 0ull};
    return cull_mask_from(L, wave_min(px), wave_min(py), wave_min(pz), wave_max(px) + ext, wave_max(py) + ext,
                          wave_max(pz) + ext);
}
__device__ __forceinline__ CullMask cull_mask_points(ModelPtr M, float px, float py, float pz, bool enable,
                                                     float ext = 0.0f) {
    if (!enable) return CullMask{0ull, 0ull};
    return cull_mask_points(load_cull_lanes(M), px, py, pz, true, ext);
}

__device__ __forceinline__ bool culled(const CullMask& cm, uint32_t i) {
    return i < 64 ? ((cm.lo >> i) & 1ull) : ((cm.hi >> (i - 64)) & 1ull);
}

// ---------------------------------------------------------------------------
// Field bounds over a box of lattice corners (k_precheck).  Most MPUs that pass S1 have
// no surface: every S2 corner is inside or every one is outside, and S2 only discards
// them (PS_Polygonizer.cpp:602-609).  An interval [lo, hi] of the field over the MPU's
// corners decides that outcome without evaluating them: hi < 0.5 (no corner inside)
// or lo >= 0.5 (no corner outside) gives exactly the reference result, 0 vertices and
// 0 triangles.  The bound is conservative by construction:
//  * each primitive's distance (Point, infinite Line, capped Cylinder, Cube: the same
//    functions the reference evaluates, all true Euclidean distances to convex sets) is
//    evaluated at the box centre and widened by what the box's half-extents allow towards
//    and away from the primitive (prim_interval, psgpu_model.h: never more than the
//    half-diagonal h); Wyvill is monotone in the distance; the field interval is widened
//    by kBoundEps, orders of magnitude above the fp32 rounding of either evaluation;
//  * ops are monotone interval maps (Blend, Union, Intersect, Dif, SmoothDif, warps);
//  * op-box pruning (depth > 3) is decided per quad of 4 z-consecutive corners: from
//    the box's exact corner coordinates the op is pruned for every quad (field 0),
//    for none (the op's interval), or for some (the interval joined with 0).
// Only models whose used primitives all have finite, well-conditioned parameters, no
// matrix, and a type above (or Triangle, field 0) are bounded (DevModel::boundable, set
// by the host; Ricci and unknown ops are excluded), so no corner can be NaN -- except a
// Cylinder on its own axis, where the bound gives up (ok = false) within 0.05 of it.
struct BoundBox {
    float cx, cy, cz, h;       // centre, half-diagonal (with margin)
    float hx, hy, hz;          // half-extents
    float xs[4], ys[4], zs[4]; // the box's corner coordinates per axis (z: one S2 quad)
};

// Field interval of one primitive over the box (TYPE: Point, Line, Cylinder or Cube): the
// interval arithmetic is prim_interval's (psgpu_model.h, host and device).
template <int TYPE, class PR>
__device__ __forceinline__ void prim_bound(PR& P, const BoundBox& B, float* lo, float* hi, bool* ok) {
    prim_interval<TYPE, PR>(P, B.cx, B.cy, B.cz, B.h, B.hx, B.hy, B.hz, lo, hi, ok);
}

// Interval of a binary op (the monotone maps of op_field; Ricci/unknown types are not bounded).
__device__ __forceinline__ void bound_op(uint32_t type, float ll, float lh, float rl, float rh, float* lo, float* hi) {
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
    default: *lo = ll; *hi = lh; break;  // warps: the left child
    }
}

// Op-box pruning of a depth > 3 op over the box's quads: a quad (x, y, 4 z) is pruned
// iff x, y and all 4 z lie outside the op box on their axes (PS_Polygonizer.cpp:1239-1243).
template <class OR>
__device__ __forceinline__ void bound_prune(OR& b, const BoundBox& B, float* lo, float* hi) {
    bool anyZ = false, allX = true, noX = true, allY = true, noY = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        anyZ = anyZ | ((B.zs[i] >= b.lo[2]) & (b.hi[2] >= B.zs[i]));
        const bool ix = (B.xs[i] >= b.lo[0]) & (b.hi[0] >= B.xs[i]);
        const bool iy = (B.ys[i] >= b.lo[1]) & (b.hi[1] >= B.ys[i]);
        allX = allX & ix; noX = noX & !ix;
        allY = allY & iy; noY = noY & !iy;
    }
    if (!anyZ && noX && noY) {  // every quad pruned: field exactly 0
        *lo = 0.0f;
        *hi = 0.0f;
    } else if (!(anyZ || allX || allY)) {  // some quads pruned
        *lo = fminf(*lo, 0.0f);
        *hi = fmaxf(*hi, 0.0f);
    }
}

// ---------------------------------------------------------------------------
// Interpreter evaluator: the flattened walk program of psgpu_model.h.
//   GROUP 4: pruning decided per 4-lane group (S1/S2 quads, S4 edge samples)
//   GROUP 1: per lane (S5: the reference evaluates 4 identical lanes)
//   COLOR  : fieldValueAndColor's colour walk as well; no subtree is skipped and lanes
//            inside a pruned subtree see field 0 for its prims and ops (the
//            reference's never-written arrays, defined as zero).
// `sl` is this lane's value stack in LDS (stride 64 floats; colour: 4 floats per slot).
struct InterpEval {
    ModelPtr M;
    float* sl;
    __device__ InterpEval(ModelPtr m, float* slots) : M(m), sl(slots) {}

    template <int GROUP, bool COLOR>
    __device__ __forceinline__ float eval(float px, float py, float pz, const CullMask& cm, float* colOut) const {
        const int n = (int)M->nInstr;
        const bool noOps = M->ctOps == 0;
        int resume = 0;
        float last = 0.0f, acc = 0.0f;
        float lc0 = 0.0f, lc1 = 0.0f, lc2 = 0.0f;
        constexpr int SW = COLOR ? 4 : 1;
        for (int pc = 0; pc < n; ++pc) {
            const Instr I = load_instr(M, pc);
            const bool act = pc >= resume;
            if (I.kind == kEnter) {
                COp& O = M->ops[I.idx];
                bool in = ((px >= O.lo[0]) & (O.hi[0] >= px)) | ((py >= O.lo[1]) & (O.hi[1] >= py)) |
                          ((pz >= O.lo[2]) & (O.hi[2] >= pz));
                bool anyIn = group_any<GROUP>(act && in);
                bool prune = act && !anyIn;
                if (prune) {
                    resume = I.skipTo;
                    sl[(I.out * SW) * 64] = 0.0f;
                    last = 0.0f;
                }
                if (!COLOR) {
                    if (ballot(pc + 1 >= resume) == 0ull) pc = I.skipTo - 1;
                }
            } else if (I.kind == kPrim) {
                if (COLOR) {
                    float f = 0.0f;
                    if (act && !culled(cm, I.idx)) f = prim_field(M->prims[I.idx], px, py, pz);
                    sl[(I.out * SW) * 64] = f;
                } else if (act) {
                    float f = 0.0f;
                    if (!culled(cm, I.idx)) f = prim_field(M->prims[I.idx], px, py, pz);
                    sl[I.out * 64] = f;
                }
            } else if (I.kind == kOp) {
                if (COLOR || act) {
                    const float lf = sl[(I.lslot * SW) * 64];
                    const float rf = sl[(I.rslot * SW) * 64];
                    float v = op_field(I.type, lf, rf, M->ops[I.idx].resY, last);
                    if (COLOR && !act) v = 0.0f;
                    sl[(I.out * SW) * 64] = v;
                    if (act) last = v;
                    if (COLOR) {
                        float cl0, cl1, cl2, cr0, cr1, cr2;
                        if (I.childKind & 2) {
                            cl0 = sl[(I.lslot * 4 + 1) * 64]; cl1 = sl[(I.lslot * 4 + 2) * 64]; cl2 = sl[(I.lslot * 4 + 3) * 64];
                        } else {
                            CPrim& P = M->prims[I.L];
                            cl0 = P.col[0]; cl1 = P.col[1]; cl2 = P.col[2];
                        }
                        if (I.childKind & 1) {
                            cr0 = sl[(I.rslot * 4 + 1) * 64]; cr1 = sl[(I.rslot * 4 + 2) * 64]; cr2 = sl[(I.rslot * 4 + 3) * 64];
                        } else {
                            CPrim& P = M->prims[I.R];
                            cr0 = P.col[0]; cr1 = P.col[1]; cr2 = P.col[2];
                        }
                        float wl, wr;
                        if (op_colour_weights(I.type, lf, rf, v, &wl, &wr)) {
                            lc0 = wl * cl0 + wr * cr0;
                            lc1 = wl * cl1 + wr * cr1;
                            lc2 = wl * cl2 + wr * cr2;
                        } else if (I.type >= 22 && I.type <= 25) {
                            lc0 = cl0; lc1 = cl1; lc2 = cl2;
                        }
                        sl[(I.out * 4 + 1) * 64] = lc0;
                        sl[(I.out * 4 + 2) * 64] = lc1;
                        sl[(I.out * 4 + 3) * 64] = lc2;
                    }
                }
            } else {  // kSumPrim
                float f = 0.0f;
                if (!culled(cm, I.idx)) f = prim_field(M->prims[I.idx], px, py, pz);
                acc = acc + f;
            }
        }
        if (COLOR) {
            if (noOps) {
                CPrim& P = M->prims[0];
                lc0 = P.col[0]; lc1 = P.col[1]; lc2 = P.col[2];
            }
            colOut[0] = lc0;
            colOut[1] = lc1;
            colOut[2] = lc2;
        }
        return noOps ? acc : last;
    }

    template <int GROUP, bool COLOR, int N>
    __device__ __forceinline__ void evaln(const float* px, const float* py, const float* pz, const CullMask& cm,
                                          float* out, float* colOut) const {
        static_assert(GROUP != 0, "the interpreter prunes per lane group, not per lane's points");
        for (int n = 0; n < N; ++n)
            out[n] = eval<GROUP, COLOR>(px[n], py[n], pz[n], cm, COLOR ? colOut + 3 * n : nullptr);
    }

    // field bounds are generated per tree (psgpu_jit.cpp); the interpreter never proves
    __device__ __forceinline__ void bound(const BoundBox&, const CullMask&, float* lo, float* hi, bool* ok) const {
        *lo = 0.0f;
        *hi = 0.0f;
        *ok = false;
    }
};

// ---------------------------------------------------------------------------
// Per-wave timeline (the reference's MPUSTATS / PrintThreadResults, PS_Polygonizer.h:201-207,
// .cpp:414-461, with waves for threads): when p.stamps is set every wave of kernel K
// records {start, end, item | hw id << 32} in the 100 MHz s_memrealtime clock, item = the
// MPU a k_mpu wave polygonized (0xffffffff: none) or the wave's global index.
__device__ __forceinline__ uint64_t stamp_now() { return __builtin_amdgcn_s_memrealtime(); }
__device__ __forceinline__ void stamp_end(const Params& p, int K, uint64_t t0, uint32_t item,
                                          const uint32_t blk = blockIdx.x) {
    const uint32_t w = blk * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= p.stampCap) return;
    const uint64_t t1 = stamp_now();
    // HW_ID (CU, SIMD, SE; 32 bits) and XCC_ID (hwreg 20) as one word: hwid[15:0] | xcc << 16
    const uint32_t hw = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);
    const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) & 15u;
    if (lane_id() == 0) {
        uint64_t* r = p.stamps + 3 * ((size_t)K * p.stampCap + w);
        r[0] = t0;
        r[1] = t1;
        r[2] = (uint64_t)item | ((uint64_t)((hw & 0xffffu) | (xcc << 16)) << 32);
    }
}
// Phase stamps inside one wave (debug bit 4096: k_mpu, 8192: k_precheck): 8 words per
// wave after the kernels' records; phase 0 = entry.
__device__ __forceinline__ void phase_stamp(const Params& p, int ph, uint32_t bit = 4096u) {
    if (!(p.debug & bit) || !p.stamps) return;
    const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= p.stampCap) return;
    const uint64_t t = stamp_now();
    if (lane_id() == 0) p.stamps[3 * (size_t)kNumStampKernels * p.stampCap + 8 * (size_t)w + ph] = t;
}
// The same, taken only once `dep` has been computed (inline asm keeps the clock read after its
// producer and in program order with the other stamps): phases of k_finish (debug bit 2048;
// the stamps change the kernel's registers, so they exist only when PSGPU_FIN_PHASES is 1).
#ifndef PSGPU_MPU_LIVE_STAMP
#define PSGPU_MPU_LIVE_STAMP 0  // k_mpu's live-primitive word: measurement builds only (PSGPU_JIT_FLAGS)
#endif
#ifndef PSGPU_FIN_PHASES
#define PSGPU_FIN_PHASES 0  // compiled in only for the measurement (PSGPU_JIT_FLAGS=-DPSGPU_FIN_PHASES=1)
#endif
__device__ __forceinline__ void phase_stamp_after(const Params& p, int ph, uint32_t bit, float dep) {
    if (!PSGPU_FIN_PHASES || !(p.debug & bit) || !p.stamps) return;
    const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= p.stampCap) return;
    uint64_t t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : "v"(dep));
    if (lane_id() == 0) p.stamps[3 * (size_t)kNumStampKernels * p.stampCap + 8 * (size_t)w + ph] = t;
}
// A kernel's span in one run (PSGPU_OPT_SPANS): every wave folds its start / end into one of
// 64 {min start, max end} pairs of the run's slot (chosen by block, so no address sees more
// than 1/64 of the waves' atomics); the host reduces the 64 pairs to the first wave start and
// the last wave end on the device clock.
__device__ __forceinline__ void span_end(const Params& p, int K, uint64_t t0) {
    const uint64_t t1 = stamp_now();
    if (lane_id() == 0) {
        uint64_t* s = p.spans + 2 * ((size_t)K * kSpanLanes + (blockIdx.x & (kSpanLanes - 1)));
        atomicMin(reinterpret_cast<unsigned long long*>(s), (unsigned long long)t0);
        atomicMax(reinterpret_cast<unsigned long long*>(s + 1), (unsigned long long)t1);
    }
}
// The reference's per-MPU MPUSTATS ticks (PS_Polygonizer.cpp:449-461: tickStart / tickEnd
// around process_cells_simd, the thread id), PSGPU_OPT_MPU_TICKS: the wave that ran S1 for
// the MPU records its start and end (k_precheck, lane g < 8 of the brick's MPU g), the wave
// that ran S2-S3 and made its vertex / triangle records raises the end (k_mpu).
__device__ __forceinline__ uint32_t wave_hw_id() {
    const uint32_t hw = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);
    const uint32_t xcc = (uint32_t)__builtin_amdgcn_s_getreg((31 << 11) | 20) & 15u;
    return (hw & 0xffffu) | (xcc << 16);
}
__device__ __forceinline__ void mpu_ticks_s1(const Params& p, uint32_t w, uint64_t t0) {
    uint64_t* r = p.mpuTicks + 4 * (size_t)w;
    r[0] = t0;
    r[1] = stamp_now();
    r[2] = 0ull;
    r[3] = (uint64_t)wave_hw_id();
}
__device__ __forceinline__ void mpu_ticks_s2(const Params& p, uint32_t m) {
    const uint64_t t = stamp_now();
    const uint32_t hw = wave_hw_id();
    if (lane_id() == 0) {
        uint64_t* r = p.mpuTicks + 4 * (size_t)(m - p.mpuBegin);
        atomicMax(reinterpret_cast<unsigned long long*>(r + 2), (unsigned long long)t);
        reinterpret_cast<uint32_t*>(r + 3)[1] = hw;
    }
}
#define PSGPU_STAMPED(K, ITEM, CALL)                                             \
    {                                                                             \
        const uint64_t t0_ = (p.stamps || p.spans) ? psgpu::stamp_now() : 0ull;  \
        uint32_t item_ = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);     \
        CALL;                                                                     \
        if (K == 1 && p.mpuTicks && ITEM != 0xffffffffu) psgpu::mpu_ticks_s2(p, ITEM); \
        if (p.stamps) psgpu::stamp_end(p, K, t0_, ITEM);                          \
        if (p.spans) psgpu::span_end(p, K, t0_);                                  \
    }

// ---------------------------------------------------------------------------
// (div_by, the exact m / d of the decodes below: psgpu_model.h)
__device__ __forceinline__ void mpu_origin(const Params& p, uint32_t m, float o[3]) {
    uint32_t k, jk;
    const uint32_t i = div_by(m, p.dims[2] * p.dims[1], p.divMagic[1], &jk);
    const uint32_t j = div_by(jk, p.dims[2], p.divMagic[0], &k);
    o[0] = p.lo[0] + (float)i * p.side;
    o[1] = p.lo[1] + (float)j * p.side;
    o[2] = p.lo[2] + (float)k * p.side;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return lane_value(wave_incl_scan(v), 63); }

// ---------------------------------------------------------------------------
// S1/S2 stages: what k_precheck, k_mpu and k_front are built from (DESIGN.md §3 "S1/S2 stages").
// Each exists once; precheck_body and mpu_body are their stage lists.  Every barrier and every
// early return between two barriers is written in the bodies, with one exception that says so in
// its name and comment: block_s2_inside_bits.

// k_front's tag of this run's queue entries: never 0 (the ready words start zeroed, and are
// zeroed again whenever the counter sets restart from epoch 0)
__device__ __forceinline__ uint32_t front_tag(const Params& p) { return p.ctr->epoch + 1u; }

// Phase word 7 of the wave's stamp row (`on`: the kernel's phase-stamp debug bit is set): its live
// primitives and, above them, what the kernel adds (S1: the lanes that passed << 16; k_mpu's
// measurement build: V << 16 | T << 32)
__device__ __forceinline__ void stamp_live_word(const Params& p, bool on, const CullMask& cm, uint64_t above) {
    if (on && p.stamps && lane_id() == 0) {
        const uint32_t w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        if (w < p.stampCap)
            p.stamps[3 * (size_t)kNumStampKernels * p.stampCap + 8 * (size_t)w + 7] =
                (uint64_t)(128 - __popcll(cm.lo) - __popcll(cm.hi)) | above;
    }
}

// Field bounds (see prim_bound): lane c of an MPU bounds the 4x4x4 corners [4X, 4X+3] x
// [4Y, 4Y+3] x [4Z, 4Z+3] of its S2 cache (its z range is exactly one S2 quad), at the S2
// coordinates (block_s2_inside_bits): o + (float)index * cs.  The one definition of the
// half-diagonal's slack, and of the half-extents': one wave-uniform value for the three axes
// and every octant of the lattice.  An octant's corners are fl(o + fl(k cs)), k = 4X .. 4X + 3,
// each within 2^-24 (|x| + 7 cs) of o + k cs, so the box reaches at most 1.5 cs + 2^-24 M from
// its true centre, M = the lattice's largest coordinate magnitude + 7 cs, and the centre as
// computed is within 2^-24 M of the true one: 1.5 cs + 2.4e-7 M covers both twice.
__device__ __forceinline__ BoundBox octant_box(const Params& p, const float o[3], int c) {
    BoundBox B;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        B.xs[i] = o[0] + (float)(4 * (c & 1) + i) * p.cs;
        B.ys[i] = o[1] + (float)(4 * ((c >> 1) & 1) + i) * p.cs;
        B.zs[i] = o[2] + (float)(4 * (c >> 2) + i) * p.cs;
    }
    const float hx = 0.5f * (B.xs[3] - B.xs[0]), hy = 0.5f * (B.ys[3] - B.ys[0]), hz = 0.5f * (B.zs[3] - B.zs[0]);
    B.cx = 0.5f * (B.xs[0] + B.xs[3]);
    B.cy = 0.5f * (B.ys[0] + B.ys[3]);
    B.cz = 0.5f * (B.zs[0] + B.zs[3]);
    B.h = __builtin_amdgcn_sqrtf(hx * hx + hy * hy + hz * hz) * 1.0001f + 1e-4f;
    float mag = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        mag = fmaxf(mag, fmaxf(fabsf(p.lo[a]), fabsf(p.lo[a] + (float)p.dims[a] * p.side)));
    B.hx = B.hy = B.hz = (1.5f * p.cs + 2.4e-7f * (mag + p.side)) * 1.0001f + 1e-4f;
    return B;
}

// The lanes' octant intervals -> bit g: MPU g passed S1 (flags8) and all 8 of its octants are
// proven outside (hi < 0.5) or all 8 inside (lo >= 0.5): no surface, 0 V / 0 T without S2.
// The two ballots stay (oct[0]: outside, oct[1]: inside; bit 8g + c: octant c of MPU g): a queued
// MPU's 16 bits go with its queue entry, and S2 walks only its undecided octants.
__device__ __forceinline__ uint32_t proven_mask(bool ok, float lo, float hi, uint32_t flags8, uint64_t oct[2]) {
    const uint64_t bOut = ballot(ok && hi < 0.5f), bIn = ballot(ok && lo >= 0.5f);
    oct[0] = bOut;
    oct[1] = bIn;
    uint32_t proven8 = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const bool all = ((bOut >> (8 * q)) & 0xffull) == 0xffull || ((bIn >> (8 * q)) & 0xffull) == 0xffull;
        proven8 |= (all ? 1u : 0u) << q;
    }
    return proven8 & flags8;
}

// Culling mask of each queued MPU (queue8; lane g < 8 holds MPU g's id in mOf), from this
// wave's culling segments (already in registers): its box grown by the normal delta, for
// k_vertex / k_finish (mpuMasks) and, with the queue entry, for S2 (k_mpu loads no culling
// data).  The grown box contains the S2 box, so its mask is conservative there too; one mask
// per MPU instead of two (the boxes differ by 0.001: the masks are the same but for primitives
// grazing the box).  Beside it the MPU's op-inside mask (op_inside_box; its own margin, no
// culling slack), lane-parallel over the ops as the culling mask is over the primitives: lane i
// holds the boxes of ops i and 64 + i, one ballot per word.  PSGPU_OPT_OP_INSIDE 0: zero masks.
// Returns to lane q < 8 MPU q's masks, for its queue entry (zero without culling).
__device__ __forceinline__ CullMask queue_masks(const Params& p, const CullLanes& cl, const float o[3],
                                                uint32_t queue8, uint32_t mOf, int lane) {
    CullMask mine{0ull, 0ull};
    if (!p.cull) return mine;
    const float eg = 7.0f * p.cs + 0.001f;
    ModelPtr Mo = as_const(p.model);
    const uint32_t nOps = p.opInside ? Mo->ctOps : 0u;
    float bl[2][3], bh[2][3];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t k = 64u * h + (uint32_t)lane;
#pragma unroll
        for (int a = 0; a < 3; ++a) {  // past ctOps: an empty box, inside of nothing
            bl[h][a] = k < nOps ? p.model->ops[k].lo[a] : 1.0f;
            bh[h][a] = k < nOps ? p.model->ops[k].hi[a] : -1.0f;
        }
    }
    for (uint32_t qm = queue8; qm != 0u; qm &= qm - 1u) {
        const int q = __builtin_ctz(qm);
        const float ox = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(o[0]), 8 * q));
        const float oy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(o[1]), 8 * q));
        const float oz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(o[2]), 8 * q));
        CullMask g = cull_mask_from(cl, ox, oy, oz, ox + eg, oy + eg, oz + eg);
        if (nOps != 0u) g.inLo = ballot((uint32_t)lane < nOps && op_inside_box(bl[0], bh[0], ox, oy, oz, p.cs));
        if (nOps > 64u)
            g.inHi = ballot(64u + (uint32_t)lane < nOps && op_inside_box(bl[1], bh[1], ox, oy, oz, p.cs));
        const uint32_t wq = lane_value(mOf, q) - p.mpuBegin;
        if (lane == 0) {
            p.mpuMasks[4 * wq] = g.lo;
            p.mpuMasks[4 * wq + 1] = g.hi;
            p.mpuMasks[4 * wq + 2] = g.inLo;
            p.mpuMasks[4 * wq + 3] = g.inHi;
        }
        if (lane == q) mine = g;
    }
    return mine;
}

// A queued MPU as S1 hands it to S2: in pq[slotq] its global id and, above it, the verdicts of
// S1's field bounds on its 8 octants (oct: bit c proven outside, bit 8 + c proven inside; zero
// without bounds; one 64-bit word, so they cost no memory instruction), and four mask words in
// pqMask[4 * slotq ..] (the MPU box's culling mask and op-inside mask, from queue_masks; not
// written and not read without culling).  Between launches (k_precheck, then k_mpu) plain
// stores and loads.  Within k_front's one launch (FRONT; MI355X_MICROARCH.md hand-off table,
// first row) S2 waves on other CUs read what S1 waves wrote: every store is write-through and
// every load agent-scope (sc1 on both sides); once a wave's entries and masks have left it
// (vmcnt(0)) each entry's ready word fqReady[slotq] takes the run's tag (publish), and an S2
// wave reads an entry only after it saw the tag there (acquire_front).
// The second op-inside word: S1 always writes it (zero for trees of at most 64 ops); the FRONT
// load skips it for such trees, the plain load takes it always -- equal values either way.
struct QueueEntry {
    uint32_t m;
    CullMask cm;
    uint32_t oct;  // S1's verdicts on the MPU's octants: bit c proven outside, bit 8 + c proven inside

    template <bool FRONT, class T>
    static __device__ __forceinline__ void put(T* at, T v) {
        if constexpr (FRONT) __hip_atomic_store(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else *at = v;
    }
    template <bool FRONT, class T>
    static __device__ __forceinline__ T get(T* at) {
        if constexpr (FRONT) return __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else return *at;
    }
    template <bool FRONT>
    __device__ __forceinline__ void store(const Params& p, uint32_t slotq) const {
        put<FRONT>(&p.pq[slotq], (uint64_t)m | ((uint64_t)oct << 32));
        if (p.cull) {
            put<FRONT>(&p.pqMask[4 * slotq], cm.lo);
            put<FRONT>(&p.pqMask[4 * slotq + 1], cm.hi);
            put<FRONT>(&p.pqMask[4 * slotq + 2], cm.inLo);
            put<FRONT>(&p.pqMask[4 * slotq + 3], cm.inHi);
        }
    }
    // FRONT only, by every lane of the wave after its stores; `mine`: this lane stored entry slotq
    static __device__ __forceinline__ void publish(const Params& p, uint32_t slotq, bool mine) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (mine) put<true>(&p.fqReady[slotq], front_tag(p));
    }
    // wave-uniform: the id and the masks in SGPRs, so every per-primitive culling test and every
    // skip of an op-box pruning test of the S2 walk is a scalar branch
    template <bool FRONT>
    static __device__ __forceinline__ QueueEntry load(const Params& p, ModelPtr M, uint32_t slotq) {
        const uint64_t id = uniform64(get<FRONT>(&p.pq[slotq]));
        QueueEntry e{(uint32_t)id, CullMask{0ull, 0ull}, (uint32_t)(id >> 32)};
        if (p.cull) {
            e.cm.lo = uniform64(get<FRONT>(&p.pqMask[4 * slotq]));
            e.cm.hi = uniform64(get<FRONT>(&p.pqMask[4 * slotq + 1]));
            e.cm.inLo = uniform64(get<FRONT>(&p.pqMask[4 * slotq + 2]));
            if (!FRONT || M->ctOps > 64u) e.cm.inHi = uniform64(get<FRONT>(&p.pqMask[4 * slotq + 3]));
        }
        return e;
    }
};

// S1: 8 corners per MPU, lanes 0-3 z = lo, lanes 4-7 z = lo + side; (x,y) lanes
// (0,0),(1,0),(0,1),(1,1) (PS_Polygonizer.cpp:488-519).  One wavefront = one 2x2x2
// brick of MPUs (lanes 8g..8g+7: MPU g = bx*4 + by*2 + bz), so the wave's culling box
// is compact.  Failing MPUs get count 0 here; survivors are appended to the sharded
// queue pq (one atomic per wave; waves [s*K, (s+1)*K) with K = pShardCap / 8 append to
// shard s, so a shard cannot overflow).  k_mpu takes them in any order: the mesh order
// comes from the scan of the per-MPU counts (in k_vertex).
// SPLIT 2 (tree split, TreeEval::kSplit): two waves per brick, one per subtree of the root
// (evaln_part / bound_part), their values exchanged through LDS and combined by both
// (combine / bound_combine): the same values, half the walk per wave -- for launches whose
// span is the heaviest brick's walk (small rank shares, a single engine).  Every wave of the
// block reaches both barriers; the second wave of a brick stops after them.
template <class EV, int SPLIT = 1, bool FRONT = false>
__device__ __forceinline__ void precheck_body(const Params& p, float* lds) {
    const int wave = (int)uniform((uint32_t)wave_index());  // scalar: so are its brick slot and tree part
    const int lane = lane_id();
    const int part = wave % SPLIT;  // subtree of the root this wave walks (SPLIT 2)
    const int slot = wave / SPLIT;  // the block's brick
    phase_stamp(p, 0, 8192u);
    const uint64_t tick0 = p.mpuTicks ? stamp_now() : 0ull;  // MPUSTATS tickStart
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // the words k_surface only ever raises (its wait's timeout, from any wave, after block 0
        // published the rest): cleared here, before any kernel of the run can raise them
        p.hostCtr->surfaceErr = 0u;
        p.totals[7] = 0u;
    }
    EV ev(as_const(p.model), lds + wave * p.slotsPerLane * 64 + lane);
    CullLanes cl;  // loaded first: independent of everything below
    if (p.cull) cl = load_cull_lanes(as_const(p.model));
    const uint32_t W = blockIdx.x * (4u / SPLIT) + (uint32_t)slot;  // brick slot: decides the queue shard
    uint32_t Wq = W;  // ... from this copy, which the split kernels keep in a vector register across
    if constexpr (SPLIT == 2) asm volatile("" : "+v"(Wq));  // the walk: they have no scalar one to spare
    const uint32_t bzN = p.brickDims[2], byN = p.brickDims[1];
    const uint32_t nBricks = p.brickDims[0] * byN * bzN;
    // The wave's brick (lattice brick coordinates).  After k_sieve: entry W of its list of live
    // bricks; a wave past the list has nothing to do (a dead brick's MPUs were written by the
    // sieve).  Otherwise brick W, or with the spreading permutation (W * brickStride) mod bricks.
    uint32_t bi, bj, bk;
    bool idle = W >= nBricks;
    if (p.sieve) {
        // written by the launch before this one: read as constants (uniform: two scalar loads, issued together)
        typedef const __attribute__((address_space(4))) uint64_t* CU64;
        typedef const __attribute__((address_space(4))) uint32_t* CU32;
        const uint64_t e = W < nBricks ? ((CU64)p.liveList)[W] : 0ull;
        idle = W >= *(CU32)&p.ctr->liveBricks;
        bi = (uint32_t)e & 0x1fffffu;
        bj = (uint32_t)(e >> 21) & 0x1fffffu;
        bk = (uint32_t)(e >> 42);
    } else {
        const uint32_t B =
            (idle || p.brickStride == 1u) ? W : (uint32_t)(((uint64_t)W * p.brickStride) % nBricks);
        uint32_t jk;
        bi = p.brickI0 + div_by(B, byN * bzN, p.brickMagic[1], &jk);
        bj = div_by(jk, bzN, p.brickMagic[0], &bk);
    }
    if (SPLIT == 1 && idle) return;  // (the split's waves stay for their block's barriers)
    const uint32_t g = (uint32_t)lane >> 3;
    const uint32_t mi = 2u * bi + ((g >> 2) & 1u);
    const uint32_t mj = 2u * bj + ((g >> 1) & 1u);
    const uint32_t mk = 2u * bk + (g & 1u);
    const uint32_t mg = (mi * p.dims[1] + mj) * p.dims[2] + mk;
    const bool valid = !idle && mi < p.dims[0] && mj < p.dims[1] && mk < p.dims[2] && mg >= p.mpuBegin &&
                       mg - p.mpuBegin < p.mpuCount;
    // A lane without an MPU of the range (a brick over the lattice's high faces or a range
    // end) takes the origin of the nearest lattice MPU, so the wave's culling box stays the
    // brick's: with MPU 0's origin there, the box of each of C3's 1,027 face bricks spans
    // the domain, every primitive stays live and those waves walk 3-5x longer (r03 timeline).
    const uint32_t ci = min(mi, p.dims[0] - 1u), cj = min(mj, p.dims[1] - 1u), ck = min(mk, p.dims[2] - 1u);
    const uint32_t m = valid ? mg : (ci * p.dims[1] + cj) * p.dims[2] + ck;
    const float o[3] = {p.lo[0] + (float)ci * p.side, p.lo[1] + (float)cj * p.side,
                        p.lo[2] + (float)ck * p.side};  // mpu_origin(m), its coordinates at hand
    const int c = lane & 7;
    const float X = (float)(c & 1), Y = (float)((c >> 1) & 1), Z = (float)(c >> 2);
    const float px = X * p.side + o[0];
    const float py = Y * p.side + o[1];
    const float pz = Z * p.side + o[2];
    // the wave's culling box: its 64 corners' (brick_box, wave-uniform: no wave reductions)
    float blo[3], bhi[3];
    brick_box(p.lo, p.side, p.dims, bi, bj, bk, blo, bhi);
    float f = -1.0f;
    CullMask cm{0ull, 0ull};
    if (p.cull) cm = cull_mask_from(cl, blo[0], blo[1], blo[2], bhi[0], bhi[1], bhi[2]);
    if constexpr (SPLIT == 2) {
        __shared__ float sF[4][64];
        float fp = -1.0f;
        if (!(p.debug & 8u) && !idle) {
            if (part == 0) ev.template evaln_part<4, false, 1, 0>(&px, &py, &pz, cm, &fp, nullptr);
            else ev.template evaln_part<4, false, 1, 1>(&px, &py, &pz, cm, &fp, nullptr);
        }
        sF[wave][lane] = fp;
        __syncthreads();
        const float rv = sF[slot * 2][lane], lv = sF[slot * 2 + 1][lane];
        if (!(p.debug & 8u)) ev.template combine<false, 1>(&rv, nullptr, &lv, nullptr, cm, &f, nullptr);
    } else if (!(p.debug & 8u)) {  // ablation bit 3: S1 without the walk (nothing passes)
        f = ev.template eval<4, false>(px, py, pz, cm, nullptr);
    } else if (p.debug & 16u) {  // bit 4: the culling mask only
        f = (float)(cm.lo & 1ull) - 1.0f;
    }
    const uint64_t bal = ballot(valid && f > 0.0f);
    phase_stamp(p, 1, 8192u);
    stamp_live_word(p, p.debug & 8192u, cm, (uint64_t)__popcll(bal) << 16);
    uint32_t flags8 = 0;  // bit g: MPU of lanes 8g..8g+7 passed
#pragma unroll
    for (int q = 0; q < 8; ++q) flags8 |= (((bal >> (8 * q)) & 0xffull) != 0ull ? 1u : 0u) << q;
    // survivors proven empty by field bounds; the wave's culling box covers every MPU of the brick
    uint32_t proven8 = 0;
    uint64_t oct[2] = {0ull, 0ull};  // the octants proven outside / inside (proven_mask); zero without bounds
    float lo = 0.0f, hi = 0.0f;  // the lane's interval over its octant
    bool ok = true;
    if ((p.debug & 1024u) && flags8 != 0u) __builtin_amdgcn_s_setprio(2);  // experiment: heavy waves first
    if constexpr (SPLIT == 2) {
        __shared__ float sLo[4][64], sHi[4][64];
        __shared__ uint32_t sOk[4][64];
        const bool doBound = p.bound && flags8 != 0u;  // the same for both waves of the brick
        if (doBound) {
            const BoundBox B = octant_box(p, o, c);
            if (part == 0) ev.template bound_part<0>(B, cm, &lo, &hi, &ok);
            else ev.template bound_part<1>(B, cm, &lo, &hi, &ok);
        }
        sLo[wave][lane] = lo;
        sHi[wave][lane] = hi;
        sOk[wave][lane] = ok ? 1u : 0u;
        __syncthreads();
        if (part != 0) return;  // the brick's first wave finishes it
        if (doBound) {
            const int r = slot * 2, l = slot * 2 + 1;
            ok = sOk[r][lane] != 0u && sOk[l][lane] != 0u;
            ev.bound_combine(sLo[r][lane], sHi[r][lane], sLo[l][lane], sHi[l][lane], cm, &lo, &hi);
            proven8 = proven_mask(ok, lo, hi, flags8, oct);
        }
    } else if (p.bound && flags8 != 0u) {
        ev.bound(octant_box(p, o, c), cm, &lo, &hi, &ok);
        proven8 = proven_mask(ok, lo, hi, flags8, oct);
        phase_stamp(p, 2, 8192u);
    }
    const uint32_t queue8 = flags8 & ~proven8;
    // lane g < 8 speaks for MPU g (its values are those of lane 8g)
    const uint32_t mOf = __shfl(m, lane * 8 & 63);
    const bool vOf = __shfl(valid ? 1 : 0, lane * 8 & 63) != 0;
    const bool pass = lane < 8 && ((queue8 >> lane) & 1u);
    if (lane < 8 && vOf) {
        // 0: failed S1; 1: passed, proven empty by field bounds; 2: passed, queued for S2
        p.passed[mOf - p.mpuBegin] = (uint8_t)(((flags8 >> lane) & 1u) + ((queue8 >> lane) & 1u));
        if (!pass) p.counts[mOf - p.mpuBegin] = 0ull;
        if (p.mpuTicks) mpu_ticks_s1(p, mOf - p.mpuBegin, tick0);
    }
    if (flags8 == 0u) return;
    const uint32_t shard = Wq / (p.pShardCap / 8u);
    if (lane == 1 && proven8 != 0u) atomicAdd(&p.ctr->shard[shard].b, (uint32_t)__popc(proven8));
    if (queue8 == 0u) return;
    // k_front: the block's sub-queue (blockIdx mod 8, the XCD of round-robin placement: a speed
    // choice only) at pq + q * fqCap, its count in shard q's p; otherwise the brick's shard
    const uint32_t qsel = FRONT ? (blockIdx.x & 7u) : shard;
    const uint32_t qbase = FRONT ? qsel * p.fqCap : shard * p.pShardCap;
    // the queue reservation's returning atomic is waited for only after the culling masks are
    // made (their round trip overlaps the mask computation; verdict r05 item 4)
    uint32_t baseAtomic = 0;
    if (lane == 0) baseAtomic = atomicAdd(&p.ctr->shard[qsel].p, (uint32_t)__popc(queue8));
    QueueEntry e{mOf, queue_masks(p, cl, o, queue8, mOf, lane), 0u};  // lane q < 8: MPU q's entry
    asm volatile("" : "+v"(baseAtomic) : "v"(e.cm.lo));  // the wait for the atomic goes here
    const uint32_t base = lane_value(baseAtomic, 0);
    const uint32_t slotq = pass ? qbase + base + (uint32_t)__popc(queue8 & ((1u << lane) - 1u)) : 0u;
    int sh = lane;  // (taken here, after the masks: made earlier, the shift is one more register across them)
    asm volatile("" : "+v"(sh) : "v"(e.cm.lo));
    sh = 8 * (sh & 7);  // lane q < 8: MPU q's octants, proven outside | proven inside << 8
    e.oct = (uint32_t)((oct[0] >> sh) & 0xffull) | ((uint32_t)((oct[1] >> sh) & 0xffull) << 8);
    if (pass) e.template store<FRONT>(p, slotq);
    phase_stamp(p, 3, 8192u);
    if constexpr (FRONT) QueueEntry::publish(p, slotq, pass);
}

// LDS per k_mpu block: one MpuLds per MPU of the block (4, or 2 with the tree split), then per
// wave the interpreter's value slots.  The S2 field values never leave registers: pass 1 needs
// only their inside bits (8 ballots, shared by the MPU's waves through LDS).
struct MpuLds {
    uint16_t edgeVid[1536];             // passes 2-3: the vertex id on each lattice edge (CellEdge::slot)
    uint8_t cfg[344];                   // per cell: its config,
    uint16_t firstV[344], firstT[344];  // ... its first vertex id and first triangle id (pass 1)
    alignas(8) uint64_t ins[8];         // the inside bits of the S2 cache
    uint32_t q[2];                      // a spare word, qt (the tree split's triangle base)
};
constexpr int kLdsMpu = (int)((sizeof(MpuLds) + 15) & ~(size_t)15);
static_assert(kLdsMpu == 4864 && __builtin_offsetof(MpuLds, ins) == 4792, "what the host sizes the launch by");
constexpr int kLdsWaveSlots = kMpusPerBlock * kLdsMpu;  // interpreter slots follow

// Last cell c in [0, 343) with first[c] <= r (first[] = exclusive prefix of per-cell
// counts, non-decreasing, first[0] = 0, so that cell holds item r): binary lifting,
// 9 fixed LDS steps.
__device__ __forceinline__ int find_cell(const uint16_t* first, uint32_t r) {
    int lo = 0;
#pragma unroll
    for (int step = 256; step > 0; step >>= 1) {
        const int mid = lo + step;
        if (mid < 343 && (uint32_t)first[mid] <= r) lo = mid;
    }
    return lo;
}

// Barrier of the MPU's waves (the whole block when the tree split gives an MPU two; LDS
// ordering within the wave when one wave does it all).
template <int WPM>
__device__ __forceinline__ void mpu_sync() {
    if (WPM > 1) {
        __syncthreads();
    } else {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// k_front: one lane waits for entry e of sub-queue q (QueueEntry's protocol) and returns its
// slot | live << 31.  Live once the ready word carries the run's tag; an entry that is still
// untagged once every S1 block of q has published (s1Done; each block counts itself after its
// waves' entries and tags left them) is past the sub-queue's end.  The wait is bounded (test
// hook PSGPU_OPT_DEBUG bit 27: a few spins against S1 blocks held back ~40 us): a broken
// protocol is flagged (error bit 4), finish re-runs as separate launches.
__device__ __forceinline__ uint32_t acquire_front(const Params& p, uint32_t q, uint32_t e) {
    const uint32_t slotq = q * p.fqCap + e, live = 0x80000000u;
    if (e >= p.fqCap) return slotq;
    const uint32_t tag = front_tag(p);
    const uint32_t need = p.preBlocks > q ? (p.preBlocks - q + 7u) / 8u : 0u;  // S1 blocks of q
    for (uint32_t spins = 0;; ++spins) {
        if (QueueEntry::get<true>(&p.fqReady[slotq]) == tag) return slotq | live;
        if ((spins & 7u) == 7u && QueueEntry::get<true>(&p.ctr->shard[q].s1Done) >= need)
            return slotq | (QueueEntry::get<true>(&p.fqReady[slotq]) == tag ? live : 0u);
        if (spins > ((p.debug & (1u << 27)) ? 8u : (1u << 22))) {
            atomicOr(&p.ctr->error, 4u);
            return slotq;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// k_mpu: the slot of the d-th queued survivor in shard order (dense over the 64 shard queues;
// sIncl: the inclusive scan of the shard counts, lane s reads shard s's), d below the total
__device__ __forceinline__ uint32_t acquire_queued(const Params& p, const uint32_t* sIncl, uint32_t d,
                                                   uint32_t incl) {
    const uint32_t pshard = (uint32_t)__popcll(ballot(incl <= d));  // first shard whose prefix passes d
    const uint32_t pidx = d - (pshard ? sIncl[pshard - 1] : 0u);
    return uniform(pshard * p.pShardCap + pidx);
}

// The tree split's S2 exchange: per wave of the block its part's values of the 8 x-slices
__device__ __forceinline__ auto s2_parts() -> float (*)[8][64] {
    __shared__ float s[4][8][64];
    return s;
}

// S2 (:550-610), block-level: every wave of the block calls it, with or without an MPU (live),
// and meets the one barrier in it (mpu_sync: the block's when the tree split gives an MPU two
// waves), between phase stamps 3 and 4.  Before it the wave's walk of the 8x8x8 corner cache of
// the MPU at o.  The field values never leave registers: pass 1 needs only their inside bits,
// ins[x] bit y*8 + z, which go through the MPU's sIns.
// One wave per MPU (SPLIT 1): only the octants S1's field bounds left undecided are walked
// (`oct`, the entry's: bit c proven outside, bit 8 + c proven inside; s2_plan_octant,
// psgpu_model.h): per pass 4 octants, 16 lanes each (lane & 3 = z', (lane >> 2) & 3 = y', the 4 x
// per lane: quads = 4 consecutive z at one (x, y), as in the full walk), one evaln<.., 4> in a
// run-time loop, so the walk's code exists once.  sIns takes the decided octants' bits as
// constants, then each pass ORs in its octants' ballots (lane 4g + n: group g's 16 bits of x
// n), all before the barrier.  PSGPU_OPT_DEBUG bit 7: every octant counts as undecided (two
// passes, all 512 corners); bit 9: the passes are counted (DevCounters::s2Passes).
// With the tree split (lane = y*8 + z, the 8 x-slices per lane; the verdicts are ignored: its
// launches are small shares where S1 weighs more) the wave walks subtree `wave % SPLIT` of the
// root, the two parts' values go through LDS and both waves combine and ballot them.
// Returns the count of inside corners; ins[] is zero without an MPU.
template <class EV, int SPLIT>
__device__ __forceinline__ uint32_t block_s2_inside_bits(EV& ev, const Params& p, bool live, const float o[3],
                                                         const CullMask& cm, uint32_t oct, int wave, uint64_t* sIns,
                                                         uint64_t ins[8]) {
    constexpr int NX = 8;  // x-slices of the S2 cache
    const int lane = lane_id();
    float fs[SPLIT > 1 ? NX : 4];  // the values of one walk: 8 x-slices, or the 4 x of an octant
    if (live) {
        const float cs = p.cs;
        phase_stamp(p, 2);
        if constexpr (SPLIT > 1) {
            const int y = lane >> 3, z = lane & 7;
            const float py = o[1] + (float)y * cs;
            const float pz = o[2] + (float)z * cs;
            float pxs[NX], pys[NX], pzs[NX];
#pragma unroll
            for (int x = 0; x < NX; ++x) {
                pxs[x] = o[0] + (float)x * cs;
                pys[x] = py;
                pzs[x] = pz;
            }
            if (wave % SPLIT == 0) ev.template evaln_part<4, false, 8, 0>(pxs, pys, pzs, cm, fs, nullptr);
            else ev.template evaln_part<4, false, 8, 1>(pxs, pys, pzs, cm, fs, nullptr);
#pragma unroll
            for (int x = 0; x < NX; ++x) s2_parts()[wave][x][lane] = fs[x];
        } else {
            const uint32_t all = (p.debug & 128u) ? 0u : 0xffffu;  // ablation: no verdict is used
            const uint32_t inside8 = (oct & all) >> 8, known = ((oct & all) | inside8) & 0xffu;
            if (lane < NX) sIns[lane] = s2_inside_const(inside8, (uint32_t)lane >> 2);
            mpu_sync<1>();  // the wave's constants are in place before its ORs
            const uint32_t passes = s2_pass_count(known);
            if ((p.debug & 512u) && lane == 0) atomicAdd(&p.ctr->s2Passes, passes);
            // The lane's plan, 8 bits per pass, in one vector register across the walks: its
            // octant, the octant of lane group lane >> 2 (lanes < 16: the ORs), that group
            // walks an octant of its own, another pass follows.  With the origin and the cell
            // size beside it the loop holds no scalar but the walk's own, and the walk's inputs
            // (the masks, as scalars, and the model's address) are opaque to the compiler in
            // each pass, so that its uniform tests and loads are made again per pass: hoisted
            // out of the loop they are all live across it (128-170 spilled SGPRs, C3 and C5).
            const uint32_t g16 = ((uint32_t)lane & 12u) << 2;  // first lane of group lane >> 2
            uint32_t plan = 0u;
#pragma unroll
            for (uint32_t t = 0; t < 2u; ++t)
                if (t < passes)
                    plan |= (s2_plan_octant(known, t, (uint32_t)lane) | (s2_plan_octant(known, t, g16) << 3) |
                             ((s2_group_walks(known, t, g16) ? 1u : 0u) << 6) | ((t + 1u < passes ? 1u : 0u) << 7))
                            << (8u * t);
            float ox = o[0], oy = o[1], oz = o[2], csv = cs;
            CullMask cml{uniform64(cm.lo), uniform64(cm.hi), uniform64(cm.inLo), uniform64(cm.inHi)};
            EV evl = ev;
            bool more = passes != 0u;
#pragma unroll 1
            while (more) {
                asm volatile("" : "+v"(plan), "+v"(ox), "+v"(oy), "+v"(oz), "+v"(csv));
                asm volatile("" : "+s"(cml.lo), "+s"(cml.hi), "+s"(cml.inLo), "+s"(cml.inHi), "+s"(evl.M));
                const uint32_t c = plan & 7u;
                const int y = 4 * (int)((c >> 1) & 1u) + ((lane >> 2) & 3), z = 4 * (int)(c >> 2) + (lane & 3);
                const float py = oy + (float)y * csv;
                const float pz = oz + (float)z * csv;
                float pxs[4], pys[4], pzs[4];
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    pxs[n] = ox + (float)(4 * (int)(c & 1u) + n) * csv;
                    pys[n] = py;
                    pzs[n] = pz;
                }
                evl.template evaln<4, false, 4>(pxs, pys, pzs, cml, fs, nullptr);
                uint64_t b = 0ull;  // lane 4g + n: the ballot of x n, for group g's 16 bits
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const uint64_t bn = ballot(fs[n] >= 0.5f);
                    if ((lane & 3) == n) b = bn;
                }
                if (lane < 16 && ((plan >> 6) & 1u)) {
                    const uint32_t cg = (plan >> 3) & 7u;
                    const uint64_t bits = s2_spread((uint32_t)(b >> g16) & 0xffffu, cg);
                    __hip_atomic_fetch_or(&sIns[4u * (cg & 1u) + ((uint32_t)lane & 3u)], bits, __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                more = uniform((plan >> 7) & 1u) != 0u;
                plan >>= 8;
            }
        }
    }
    phase_stamp(p, 3);
    mpu_sync<SPLIT>();
    phase_stamp(p, 4);
    uint32_t inside = 0;
#pragma unroll
    for (int x = 0; x < NX; ++x) ins[x] = SPLIT == 1 && live ? sIns[x] : 0ull;
    if constexpr (SPLIT > 1) {
        if (live) {
            const int first = wave / SPLIT * SPLIT;  // the MPU's first wave
            float rv[NX], lv[NX];
#pragma unroll
            for (int x = 0; x < NX; ++x) {
                rv[x] = s2_parts()[first][x][lane];
                lv[x] = s2_parts()[first + 1][x][lane];
            }
            ev.template combine<false, 8>(rv, nullptr, lv, nullptr, cm, fs, nullptr);
#pragma unroll
            for (int x = 0; x < NX; ++x) ins[x] = ballot(fs[x] >= 0.5f);
        }
    }
#pragma unroll
    for (int x = 0; x < NX; ++x) inside += __popcll(ins[x]);
    return inside;
}

// S3 pass 1 (:647-691): config per cell (bit c = x*4 + y*2 + z, inside = f >= 0.5),
// owned sign-changing edges (new vertices) and triangles; wave prefix sums give
// the reference's discovery order over cells (i,j,k): one x-slab i per step, lane
// j*8 + k, so the cell's corners are bits lane + {0, 1, 8, 9} of ins[i] and ins[i+1].
// Every wave of the MPU computes the counts; the first writes the tables (per cell its
// config and its first vertex and triangle ids).  Returns V | T << 16 (both <= 343 * 12
// per MPU: no carry between the halves).
__device__ __forceinline__ uint32_t count_cells(const CubeTablesDev* tab, const uint64_t ins[8], bool first,
                                                MpuLds& L) {
    const int lane = lane_id();
    uint32_t carry = 0;
    const int j = lane >> 3, k = lane & 7;
    const bool cellLane = j < 7 && k < 7;
    const uint32_t ownJK = tab->own[(j == 0 ? 2 : 0) | (k == 0 ? 1 : 0)];    // cells with i > 0
    const uint32_t ownJK0 = tab->own[4 | (j == 0 ? 2 : 0) | (k == 0 ? 1 : 0)];  // the i == 0 slab
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const int c = i * 49 + j * 7 + k;
        const uint32_t b0 = (uint32_t)(ins[i] >> lane), b1 = (uint32_t)(ins[i + 1] >> lane);
        uint32_t cfg = 0;
        if (cellLane) cfg = (b0 & 3u) | ((b0 >> 6) & 12u) | ((b1 & 3u) << 4) | (((b1 >> 8) & 3u) << 6);
        uint32_t nvt = 0;
        if (cfg != 0 && cfg != 255) {
            const uint32_t cn = tab->crossNtri[cfg];
            nvt = (uint32_t)__popc((i == 0 ? ownJK0 : ownJK) & cn & 0xfffu) | (cn & 0xffff0000u);
        }
        const uint32_t svt = wave_incl_scan(nvt);  // one scan for both counts
        if (cellLane && first) {
            const uint32_t id = carry + svt - nvt;
            L.cfg[c] = (uint8_t)cfg;
            L.firstV[c] = (uint16_t)(id & 0xffffu);
            L.firstT[c] = (uint16_t)(id >> 16);
        }
        carry += lane_value(svt, 63);
    }
    return carry;
}

// Block reservation (block-level: the three steps of one rendezvous over these shared words).
// The block reserves its vertex records with one atomic into shard blk & 63, its MPUs back to
// back (the 64-record batches of k_vertex / k_finish then straddle MPUs of one S1 brick, whose
// live primitive sets overlap: DESIGN.md §4).  reset: before the prologue's barrier, which every
// wave of the block reaches.  arrive: one lane per MPU, after S3 pass 1, leaves its V (0 without
// surface) in slot order and counts itself in; the last to arrive has all of them and reserves
// their sum.  Its wait for the atomic is the block's: the base is published at the barrier that
// follows (making each wave's first batch of records before the barrier, to hide that wait,
// measured the same: profiles/r07_block_reserve_ab.txt).  base_of: after that barrier, the
// block's base + the V of the earlier slots.
template <int MPB>
struct BlockReserve {
    uint32_t v[MPB], arrived, base;
    __device__ __forceinline__ void reset() { arrived = 0u; }  // by one thread
    __device__ __forceinline__ void arrive(const Params& p, uint32_t blk, int slot, uint32_t V) {
        v[slot] = V;
        if (__hip_atomic_fetch_add(&arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP) == MPB - 1u) {
            uint32_t sum = 0;
#pragma unroll
            for (int k = 0; k < MPB; ++k) sum += v[k];
            base = sum ? atomicAdd(&p.ctr->shard[blk & (kShards - 1)].v, sum) : 0u;
        }
    }
    __device__ __forceinline__ uint32_t base_of(int slot) const {
        uint32_t qv = base;
#pragma unroll
        for (int k = 0; k < MPB - 1; ++k)
            if (k < slot) qv += v[k];
        return qv;
    }
};

// The decodes passes 2 and 3 share (if they disagreed, pass 3 would read an edgeVid slot that
// pass 2 did not write): cell c -> (i, j, k), and edge ed of that cell -> the lattice edge it
// is (CellEdge): low corner (sx, sy, sz) of the 8x8x8 cache and axis, from the table's edgeBits.
struct CellIjk {
    int i, j, k;
};
__device__ __forceinline__ CellIjk cell_ijk(int c) { return CellIjk{c / 49, (c / 7) % 7, c % 7}; }
struct CellEdge {
    int sx, sy, sz, ax;
    __device__ __forceinline__ CellEdge(uint64_t edgeBits, const CellIjk& c, int ed) {
        const int eb = (int)((edgeBits >> (5 * ed)) & 31u), c1 = eb & 7;
        sx = c.i + ((c1 >> 2) & 1), sy = c.j + ((c1 >> 1) & 1), sz = c.k + (c1 & 1), ax = eb >> 3;
    }
    __device__ __forceinline__ int slot() const { return ((sx * 8 + sy) * 8 + sz) * 3 + ax; }  // in edgeVid
};

// pass 2 (:703-762), one lane per new vertex r (batches of 64 dealt to the MPU's waves
// in turn): its cell is the last cell whose first vertex id is <= r; it is that cell's
// k-th owned crossing edge in first-occurrence order of the row, k = r - first id.
// Records are written coalesced, from qv (BlockReserve::base_of) on.
template <int WPM>
__device__ __forceinline__ void vertex_records(const Params& p, uint64_t edgeBits, MpuLds& L, VertexKey* vk,
                                               uint32_t w, uint32_t V, uint32_t qv, int part) {
    const CubeTablesDev* tab = p.tables;
    const int lane = lane_id();
    for (uint32_t b0 = (uint32_t)part * 64u; b0 < V; b0 += 64u * WPM) {
        const uint32_t r = b0 + (uint32_t)lane;
        if (r < V) {
            const int c = find_cell(L.firstV, r);
            const uint32_t cfg = L.cfg[c];
            const CellIjk at = cell_ijk(c);
            const uint32_t own = tab->own[(at.i == 0 ? 4 : 0) | (at.j == 0 ? 2 : 0) | (at.k == 0 ? 1 : 0)];
            const uint64_t order = tab->order[cfg];
            uint32_t left = r - L.firstV[c];
            int ed = 0;
            for (int q = 0; q < 12; ++q) {  // the (left+1)-th owned edge of the row order
                ed = (int)((order >> (4 * q)) & 15u);
                if ((own >> ed) & 1u) {
                    if (left == 0u) break;
                    --left;
                }
            }
            const CellEdge e(edgeBits, at, ed);
            L.edgeVid[e.slot()] = (uint16_t)r;
            const uint32_t key = (uint32_t)e.sx | ((uint32_t)e.sy << 3) | ((uint32_t)e.sz << 6) | ((uint32_t)e.ax << 9);
            const uint32_t g = qv + r;
            if (g < p.vShardCap) vk[g] = VertexKey{w, r | (key << 16)};
        }
    }
}

// pass 3 (S6, :816-825), one lane per triangle r: its cell (last first-id <= r) and
// the (r - first)-th triangle of the cell's table row; records from qt on
template <int WPM>
__device__ __forceinline__ void triangle_records(const Params& p, uint64_t edgeBits, const MpuLds& L, TriRec* tq,
                                                 uint32_t w, uint32_t T, uint32_t qt, int part) {
    const int lane = lane_id();
    for (uint32_t b0 = (uint32_t)part * 64u; b0 < T; b0 += 64u * WPM) {
        const uint32_t r = b0 + (uint32_t)lane;
        if (r < T) {
            const int c = find_cell(L.firstT, r);
            const uint32_t t = r - L.firstT[c];
            const CellIjk at = cell_ijk(c);
            const uint64_t row = p.tables->row[L.cfg[c]];
            uint32_t v[3];
#pragma unroll
            for (int sv = 0; sv < 3; ++sv) {
                const int ed = (int)((row >> (4 * (t * 3 + sv))) & 15u);
                v[sv] = L.edgeVid[CellEdge(edgeBits, at, ed).slot()];
            }
            const uint32_t g = qt + r;
            if (g < p.tShardCap)
                tq[g] = TriRec{r | ((v[2] >> 10) << 11) | ((w >> 6) << 12), v[0] | (v[1] << 11) | ((v[2] & 1023u) << 22)};
        }
    }
}

// Per-MPU body: one wavefront per MPU that passed S1 (and was not proven empty), 4
// wavefronts per block.  Every wave of a block reaches every barrier: waves without an MPU
// (past the last survivor) or whose MPU has no surface just skip the work.
// SPLIT 2 (tree split): two waves per MPU, each walking one subtree of the root over all
// 8 x-slices (evaln_part), the values exchanged through LDS and combined by both waves
// (combine), which then share the record passes (batches of 64 records dealt in turn).
// FRONT (k_front, the S2 blocks of the launch whose first p.preBlocks blocks run S1): block blk
// takes entries [MPB * (blk >> 3), MPB * (blk >> 3) + MPB) of sub-queue blk & 7 as their S1
// waves publish them (their ready words carry the run's tag), instead of the d-th survivor
// of the finished shard queues; an entry that is still untagged once every S1 block of its
// sub-queue has published is past the sub-queue's end.
template <class EV, int SPLIT = 1, bool FRONT = false>
__device__ __forceinline__ void mpu_body(const Params& p, unsigned char* smem, uint32_t* item,
                                         const uint32_t blk = blockIdx.x) {
    *item = 0xffffffffu;
    constexpr int WPM = SPLIT;     // waves per MPU
    constexpr int MPB = 4 / SPLIT;  // MPUs per block
    const int wave = wave_index();
    const int lane = lane_id();
    const int slot = wave / WPM;  // the block's MPU this wave works on
    const int part = wave % WPM;  // its subtree of the root (SPLIT 2), and its turn in the record passes
    phase_stamp(p, 0);
    uint32_t d = blk * (uint32_t)MPB + (uint32_t)slot;
    ModelPtr M = as_const(p.model);
    const CubeTablesDev* tab = p.tables;  // global: L1 / L2 resident (an LDS copy per block measured slower, r05)
    bool live;
    uint32_t slotq = 0;
    __shared__ BlockReserve<MPB> sRes;
    if (threadIdx.x == 0) sRes.reset();
    if constexpr (FRONT) {
        const uint32_t q = blk & 7u, e = (blk >> 3) * (uint32_t)MPB + (uint32_t)slot;
        d = (e << 3) | q;  // spreads the MPU's vertex records over the shards
        __shared__ uint32_t sFront[4];  // per MPU of the block: entry | live << 31
        if (part == 0 && lane == 0) sFront[slot] = acquire_front(p, q, e);
        __syncthreads();  // the MPU's other wave reads the entry after the barrier its poller joined
        bool any = false;
#pragma unroll
        for (int k = 0; k < MPB; ++k) any |= (sFront[k] >> 31) != 0u;
        if (!any) return;  // no entry for this block (block-uniform)
        slotq = sFront[slot] & 0x7fffffffu;
        live = (sFront[slot] >> 31) != 0u;
    } else {
        // prologue: wave 0 reads the 64 shard counts (one 128-B line each) and scans them for
        // the block
        __shared__ uint32_t sIncl[kShards];
        if (wave == 0) {
            const uint32_t cnt = p.ctr->shard[lane].p;  // kShards == 64: one shard per lane
            sIncl[lane] = wave_incl_scan(cnt);
        }
        __syncthreads();
        // the grid is sized by the host from the last finished run, and a run with more
        // survivors than that is re-run by finish()
        const uint32_t incl = sIncl[lane];
        const uint32_t pcount = sIncl[kShards - 1];
        if (blk * (uint32_t)MPB >= pcount) return;  // whole block past the last survivor
        live = d < pcount;
        if (live) slotq = acquire_queued(p, sIncl, d, incl);
    }
    QueueEntry e{0u, CullMask{0ull, 0ull}};
    uint32_t w = 0;
    float o[3] = {0.0f, 0.0f, 0.0f};
    if (live) {
        e = QueueEntry::load<FRONT>(p, M, slotq);
        *item = e.m;
        w = e.m - p.mpuBegin;  // slot of the MPU in the range: counts / offsets index
        mpu_origin(p, e.m, o);
    }
    phase_stamp(p, 1);
    MpuLds& L = *reinterpret_cast<MpuLds*>(smem + slot * kLdsMpu);
    EV ev(M, reinterpret_cast<float*>(smem + kLdsWaveSlots + wave * p.slotsPerLane * 64 * 4) + lane);
    uint64_t ins[8];  // (block-level: the S2 barrier is in it)
    const uint32_t inside = block_s2_inside_bits<EV, SPLIT>(ev, p, live, o, e.cm, e.oct, wave, L.ins, ins);
    const bool work = live && inside != 0 && inside != 512 && !(p.debug & 1u);
    if (live && !work && part == 0 && lane == 0) p.counts[w] = 0ull;  // no vertices, no triangles

    const uint64_t edgeBits = tab->edge;
    uint32_t V = 0, T = 0;
    // WPM 1: the triangle queue's base stays in lane 0's registers (the returning atomic is not
    // waited for until pass 3 reads it: its round trip overlaps pass 2; verdict r05 item 4: the
    // record passes hold half of k_mpu's parked cycles)
    uint32_t qtAtomic = 0u;
    if (work) {
        const uint32_t vt = count_cells(tab, ins, part == 0, L);
        V = vt & 0xffffu;
        T = vt >> 16;
        if (part == 0) {
            const uint32_t shard = d & (kShards - 1);
            if (lane == 0) {
                qtAtomic = atomicAdd(&p.ctr->shard[w & (kShards - 1)].t, T);  // TriRec: shard = w & 63
                if (WPM > 1) L.q[1] = qtAtomic;
                p.counts[w] = (uint64_t)V | ((uint64_t)T << 32);
                if (T > 0) atomicAdd(&p.ctr->shard[shard].s, 1u);
                if (V > 512u || T > 512u) atomicMin(&p.ctr->firstOverflow, (int)e.m);
            }
        }
    }
    phase_stamp(p, 5);
#if PSGPU_MPU_LIVE_STAMP
    // measurement builds only: the MPU's V and T beside the wave's live primitives
    if (live) stamp_live_word(p, p.debug & 4096u, e.cm, ((uint64_t)V << 16) | ((uint64_t)T << 32));
#endif
    const bool recs = work && !(p.debug & 2u);  // ablation bit 1: pass 1 only
    if (part == 0 && lane == 0) sRes.arrive(p, blk, slot, V);
    __syncthreads();
    if (WPM == 1 && !work) return;
    VertexKey* vk = p.vk + (size_t)(blk & (kShards - 1)) * p.vShardCap;
    TriRec* tq = p.tq + (size_t)(w & (kShards - 1)) * p.tShardCap;
    if (recs) vertex_records<WPM>(p, edgeBits, L, vk, w, V, sRes.base_of(slot), part);
    phase_stamp(p, 6);
    mpu_sync<WPM>();
    if (!recs || (p.debug & 4u)) return;  // ablation bit 2: no triangles
    const uint32_t qt = WPM > 1 ? L.q[1] : lane_value(qtAtomic, 0);
    triangle_records<WPM>(p, edgeBits, L, tq, w, T, qt, part);
}

// Batches of `per` records over the kShards queues: lane l holds shard l's batch
// count, so a batch index maps to (shard, first record) with one ballot.
// The block's copy of the 64 shard counts of one ShardCtr field (word `field`): the first
// 64 threads gather the 64 lines once per block; the caller syncs the block before use.
__device__ __forceinline__ void stage_shard_counts(const Params& p, int field, uint32_t* s) {
    if (threadIdx.x < (unsigned)kShards)
        s[threadIdx.x] = reinterpret_cast<const uint32_t*>(&p.ctr->shard[threadIdx.x])[field];
}

struct ShardBatches {
    uint32_t cnt, incl, total;
    __device__ ShardBatches(const uint32_t* staged, uint32_t cap, uint32_t per) {
        cnt = min(staged[lane_id()], cap);  // staged by stage_shard_counts
        const uint32_t nb = (cnt + per - 1) / per;
        incl = wave_incl_scan(nb);
        total = lane_value(incl, kShards - 1);
        perBatch = per;
        nbat = nb;
    }
    uint32_t perBatch, nbat;
    __device__ void locate(uint32_t b, uint32_t* shard, uint32_t* first, uint32_t* count) const {
        const uint32_t s = (uint32_t)__popcll(ballot(incl <= b));
        const uint32_t start = __shfl(incl - nbat, (int)s);
        *shard = s;
        *first = (b - start) * perBatch;
        *count = __shfl(cnt, (int)s);
    }
};

// Exclusive offsets of the per-MPU (V | T << 32) counts of the range, in MPU order (the
// reference's PolyMPUs order): offs[0] = 0, offs[w + 1] = inclusive sum.  Single pass,
// run by the first scanBlocks 256-thread blocks of k_vertex (all co-resident): each owns
// chunks of kScanItems counts (8 consecutive per thread, 64-B vector loads), publishes
// its aggregate, looks back over up to 64 predecessors at once (decoupled look-back),
// then scans.  V and T halves are scanned as two u32 DPP
// scans (their totals stay below 2^31).  Status words (state << 62 | T << 31 | V) start
// at zero: the previous run's k_finish cleared them.  All blocks are resident.
__device__ __forceinline__ uint64_t scan_word(uint32_t state, uint32_t v, uint32_t t) {
    return ((uint64_t)state << 62) | ((uint64_t)(t & 0x7fffffffu) << 31) | (uint64_t)(v & 0x7fffffffu);
}

struct Chunk8 {
    uint64_t c[8];
    __device__ void load(const uint64_t* counts, uint32_t e, uint32_t hi) {
        if (e + 8 <= hi) {
            const uint4* src = reinterpret_cast<const uint4*>(counts + e);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4 q = src[i];
                c[2 * i] = (uint64_t)q.x | ((uint64_t)q.y << 32);
                c[2 * i + 1] = (uint64_t)q.z | ((uint64_t)q.w << 32);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) c[i] = e + i < hi ? counts[e + i] : 0ull;
        }
    }
    __device__ void sum(uint32_t& v, uint32_t& t) const {
        v = 0u;
        t = 0u;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v += (uint32_t)c[i];
            t += (uint32_t)(c[i] >> 32);
        }
    }
};

__device__ __forceinline__ void scan_counts_block(const Params& p, uint32_t b) {
    constexpr int kWaves = (int)(kScanItems / 512u);
    __shared__ uint32_t sWave[2][kWaves];
    __shared__ uint32_t sPrefix[2];
    const uint32_t n = p.mpuCount;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const uint32_t lo = b * p.scanChunks * kScanItems;
    const uint32_t hi = min(n, lo + p.scanChunks * kScanItems);
    // pass 1: the block's aggregate (the first chunk stays in registers)
    Chunk8 ch;
    ch.load(p.counts, lo + (uint32_t)t * 8u, hi);
    uint32_t sv, st;
    ch.sum(sv, st);
    for (uint32_t c = 1; c < p.scanChunks; ++c) {
        Chunk8 more;
        more.load(p.counts, lo + c * kScanItems + (uint32_t)t * 8u, hi);
        uint32_t a, bb;
        more.sum(a, bb);
        sv += a;
        st += bb;
    }
    const uint32_t wv_v = lane_value(wave_incl_scan(sv), 63), wv_t = lane_value(wave_incl_scan(st), 63);
    if (lane == 0) {
        sWave[0][wv] = wv_v;
        sWave[1][wv] = wv_t;
    }
    __syncthreads();
    if (wv == 0) {
        uint32_t aggV = 0u, aggT = 0u;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            aggV += sWave[0][w];
            aggT += sWave[1][w];
        }
        uint32_t exV = 0u, exT = 0u;
        if (b == 0) {
            if (lane == 0) __hip_atomic_store(&p.scanStatus[0], scan_word(2, aggV, aggT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (lane == 0) __hip_atomic_store(&p.scanStatus[b], scan_word(1, aggV, aggT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int64_t j = (int64_t)b - 1;
            for (;;) {
                const int64_t idx = j - lane;
                uint32_t state = 2, v = 0u, tt = 0u;
                if (idx >= 0) {
                    uint64_t w = 0ull;
                    uint32_t spins = 0;  // bounded: a broken protocol ends the kernel, flagged
                    do {
                        w = __hip_atomic_load(&p.scanStatus[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } while ((w >> 62) == 0ull && ++spins < (1u << 20));
                    if (p.debug & (1u << 26)) w = 0ull;  // test hook: every look-back times out
                    if ((w >> 62) == 0ull) {
                        atomicOr(&p.ctr->error, 1u);
                        w = scan_word(2, 0u, 0u);
                    }
                    state = (uint32_t)(w >> 62);
                    v = (uint32_t)(w & 0x7fffffffull);
                    tt = (uint32_t)((w >> 31) & 0x7fffffffull);
                }
                const uint64_t inc = ballot(state == 2);
                const bool stop = inc != 0ull;
                const int k = stop ? __builtin_ctzll(inc) : 63;  // newest predecessor with an inclusive prefix
                exV += lane_value(wave_incl_scan(lane <= k ? v : 0u), 63);
                exT += lane_value(wave_incl_scan(lane <= k ? tt : 0u), 63);
                if (stop) break;
                j -= 64;
            }
            if (lane == 0)
                __hip_atomic_store(&p.scanStatus[b], scan_word(2, exV + aggV, exT + aggT), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
            sPrefix[0] = exV;
            sPrefix[1] = exT;
        }
    }
    if (b == 0 && t == 0) p.offs[0] = 0ull;
    __syncthreads();
    // pass 2: per thread 8 consecutive counts; one block-wide scan per chunk
    uint32_t carryV = sPrefix[0], carryT = sPrefix[1];
    for (uint32_t c = 0; c < p.scanChunks; ++c) {
        const uint32_t e0 = lo + c * kScanItems + (uint32_t)t * 8u;
        if (c > 0) {
            ch.load(p.counts, e0, hi);
            ch.sum(sv, st);
            __syncthreads();  // sWave reuse
        }
        const uint32_t iv = wave_incl_scan(sv), it = wave_incl_scan(st);
        if (lane == 63) {
            sWave[0][wv] = iv;
            sWave[1][wv] = it;
        }
        __syncthreads();
        uint32_t runV = carryV + iv - sv, runT = carryT + it - st;
        uint32_t totV = 0u, totT = 0u;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint32_t a = sWave[0][w], bb = sWave[1][w];
            runV += w < wv ? a : 0u;
            runT += w < wv ? bb : 0u;
            totV += a;
            totT += bb;
        }
        uint64_t out[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            runV += (uint32_t)ch.c[i];
            runT += (uint32_t)(ch.c[i] >> 32);
            out[i] = (uint64_t)runV | ((uint64_t)runT << 32);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (e0 + i < hi) p.offs[e0 + i + 1] = out[i];
        carryV += totV;
        carryT += totT;
    }
}

// Culling mask of a wave whose lanes hold points of the MPUs w (range slots): the AND of
// those MPUs' masks (k_mpu, box grown by the normal delta), one scalar load pair per
// distinct MPU.  A primitive culled for every one of the boxes is +0 at all the points; the
// op-inside words alike: inside an op's box for every MPU's box is inside for every point.
__device__ __forceinline__ CullMask cull_mask_mpus(const Params& p, uint32_t w) {
    CullMask cm{~0ull, ~0ull, ~0ull, ~0ull};
    bool todo = true;
    for (;;) {
        const uint64_t b = ballot(todo);
        if (b == 0ull) break;
        const uint32_t w0 = lane_value(w, (int)__builtin_ctzll(b));
        cm.lo &= p.mpuMasks[4 * w0];
        cm.hi &= p.mpuMasks[4 * w0 + 1];
        cm.inLo &= p.mpuMasks[4 * w0 + 2];
        cm.inHi &= p.mpuMasks[4 * w0 + 3];
        if (w == w0) todo = false;
    }
    return cm;
}

// The edge of a vertex record (PS_Polygonizer.cpp:722-724): e1 = lo + cs*s, e2 = e1 with
// e2[axis] += cs, d = e2 - e1, and its samples e1 + d * (l/3), l = 0..3 (:744-755).  k_vertex
// brackets the root with them; k_finish recomputes the root from the record (iv, scale)
// through the same expressions, so both kernels see the same bits.
struct EdgeSeg {
    float e[3], d[3];
};
__device__ __forceinline__ EdgeSeg edge_segment(const Params& p, uint32_t w, uint32_t key) {
    float o[3];
    mpu_origin(p, w + p.mpuBegin, o);  // the MPU origin, as k_mpu computed it
    const int sx = key & 7, sy = (key >> 3) & 7, sz = (key >> 6) & 7, ax = (key >> 9) & 3;
    const float cs = p.cs;
    EdgeSeg E;
    E.e[0] = o[0] + cs * (float)sx;
    E.e[1] = o[1] + cs * (float)sy;
    E.e[2] = o[2] + cs * (float)sz;
    E.d[0] = (ax == 0 ? E.e[0] + cs : E.e[0]) - E.e[0];
    E.d[1] = (ax == 1 ? E.e[1] + cs : E.e[1]) - E.e[1];
    E.d[2] = (ax == 2 ? E.e[2] + cs : E.e[2]) - E.e[2];
    return E;
}
__device__ __forceinline__ float edge_sample(float e, float d, int l) {
    const float third = 1.0f / 3.0f;
    return e + d * ((float)l * third);
}
// the linear root on [sample iv - 1, sample iv] (:756-762): a + scale * (b - a)
__device__ __forceinline__ void vertex_root(const EdgeSeg& E, uint32_t iv, float scale, float pos[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a = edge_sample(E.e[c], E.d[c], (int)iv - 1);
        const float b = edge_sample(E.e[c], E.d[c], (int)iv);
        pos[c] = a + scale * (b - a);
    }
}

// ---------------------------------------------------------------------------
// Vertex stages.  k_vertex, k_finish and k_surface are compositions of the stages below; each
// stage exists once, templated on the evaluator and, where the layout matters, on the
// vertices per wave (VPW):
//   VPW 16 (quad): 4 lanes per vertex, one point of a walk per lane;
//   VPW 32 (pair): 2 lanes per vertex, two points per lane (shading only);
//   VPW 64 (wide): one lane per vertex, its 4 points as one walk.
// The fewer vertices a wave holds, the shorter its walk: the narrow layouts serve launches
// whose vertices do not fill the persistent grid (a small rank share), the wide one has more
// total throughput (packed fp32, one set of uniform work per 4 points) and serves large runs.
// The launch plan chooses; every layout computes the same bits.

// Stage: the vertex record of a lane.  Batch `batch` of the shard queues holds VPW records, one
// per group of 64 / VPW lanes.  Lanes past the shard's count take the batch's first record, so
// that every lane walks a real point, and drop their results (`valid`).
struct VertexSlot {
    size_t rec;  // index into p.vk / p.vp
    bool valid;
    int j;  // the lane's position in its vertex's lane group
};
template <int VPW>
__device__ __forceinline__ VertexSlot locate_vertex(const Params& p, const ShardBatches& sb, uint32_t batch) {
    constexpr int kLanes = 64 / VPW;  // lanes per vertex
    uint32_t shard, first, count;
    sb.locate(batch, &shard, &first, &count);
    uint32_t rr = first + (uint32_t)(lane_id() / kLanes);
    const bool valid = rr < count;
    if (!valid) rr = first;
    return VertexSlot{(size_t)shard * p.vShardCap + rr, valid, lane_id() & (kLanes - 1)};
}

// The quad layouts' exchange: every lane of a quad gets the value of each of its 4 lanes.
__device__ __forceinline__ void quad_gather(float v, float out[4]) {
    out[0] = quad_bcast<0>(v);
    out[1] = quad_bcast<1>(v);
    out[2] = quad_bcast<2>(v);
    out[3] = quad_bcast<3>(v);
}

// The MPU culling mask of a wave's edge samples: every sample lies in its MPU's box (k_mpu's
// mask; the d^2 >= 1.02 margin absorbs the last-bit rounding of e1 + cs vs lo + 7 cs).
__device__ __forceinline__ CullMask edge_mask(const Params& p, uint32_t w) {
    return p.cull ? cull_mask_mpus(p, w) : CullMask{0ull, 0ull};
}

// Stage: the root's bracket (PS_Polygonizer.cpp:744-755).  The field at the edge's 4 samples,
// then the first sample whose inside state differs from sample 0, else 3, and the linear
// root's scale on [sample iv - 1, sample iv]; vertex_root makes the position from the two.
// Quad: lane j walks sample j, op-box pruning decided per quad (GROUP 4), the 4 values gathered
// over DPP.  Wide: the lane's 4 samples as one 4-point walk whose pruning groups the lane's 4
// points (GROUP 0) as the quad layout groups the quad's lanes.
template <class EV, int VPW>
__device__ __forceinline__ VertexPos root_bracket(EV& ev, const Params& p, const EdgeSeg& E, const CullMask& cm,
                                                  const VertexSlot& s) {
    static_assert(VPW == 16 || VPW == 64, "the root walks one or four samples per lane");
    float fs[4];
    if constexpr (VPW == 64) {
        float xs[4], ys[4], zs[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            xs[l] = edge_sample(E.e[0], E.d[0], l);
            ys[l] = edge_sample(E.e[1], E.d[1], l);
            zs[l] = edge_sample(E.e[2], E.d[2], l);
        }
        if (p.debug & 256u) {  // ablation bit 8: no phase-A walk
#pragma unroll
            for (int l = 0; l < 4; ++l) fs[l] = xs[l];
        } else {
            ev.template evaln<0, false, 4>(xs, ys, zs, cm, fs, nullptr);
        }
    } else {
        const float qx = edge_sample(E.e[0], E.d[0], s.j);
        const float qy = edge_sample(E.e[1], E.d[1], s.j);
        const float qz = edge_sample(E.e[2], E.d[2], s.j);
        float f;
        if (p.debug & 256u) f = qx;  // ablation bit 8: no phase-A walk
        else f = ev.template eval<4, false>(qx, qy, qz, cm, nullptr);
        quad_gather(f, fs);
    }
    const bool st0 = fs[0] >= 0.5f;
    const int iv = ((fs[1] >= 0.5f) != st0) ? 1 : (((fs[2] >= 0.5f) != st0) ? 2 : 3);
    const float fa = iv == 1 ? fs[0] : (iv == 2 ? fs[1] : fs[2]);
    const float fb = iv == 1 ? fs[1] : (iv == 2 ? fs[2] : fs[3]);
    return VertexPos{(0.5f - fa) / (fb - fa), (uint32_t)iv};
}

// Stage: colour and unit normal at the root P.  fieldValueAndColor's value and colour walk at P
// (PS_Polygonizer.cpp:777-778, 1378-1551) and the normal's per-point fieldValue at
// P + delta e_x, P + delta e_y, P + delta e_z (:780-781, 1598-1622) are four points of one
// colour walk with per-point pruning (GROUP 1; the colour of points 1-3 is dead code), then
// the normal -(f(P + delta e_a) - f(P)) / delta and SimdNormalize (rsqrt -> IEEE 1/sqrtf).
// Quad: lane j walks point j.  Pair: lane j walks points 2j and 2j + 1 and takes its partner's
// over DPP.  Wide: all four in one lane.  Every lane of a vertex ends with all of S.
// Culling: a wave whose roots all lie on their bracketing segments (inside their MPUs' boxes;
// no inf / NaN) takes the MPU masks, whose boxes are grown by delta and so cover every normal
// sample; any other wave the box of its own points grown by delta.  `mpuMask` is called only in
// the first case: k_finish loads the masks there, k_surface hands over the bracket's.
// STAMP (k_finish's wide loop under PSGPU_FIN_PHASES): phases 3, 4 and word 7 for tools/timeline.py.
struct Shaded {
    float c[3], n[3];
};
template <class EV, int VPW, bool STAMP = false, class MPUMASK>
__device__ __forceinline__ Shaded shade_vertex(EV& ev, const Params& p, const float P[3], bool onSeg,
                                               const VertexSlot& s, MPUMASK mpuMask) {
    const float delta = 0.001f;
    const float inv = -1.0f / delta;
    Shaded S{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
    if (p.debug & 32u) return S;  // ablation bit 5: no walks
    CullMask cm{0ull, 0ull};
    if (p.cull) {
        if (ballot(!onSeg) == 0ull) cm = mpuMask();
        else cm = cull_mask_points(as_const(p.model), P[0], P[1], P[2], true, delta);
    }
    if constexpr (STAMP) {
        phase_stamp_after(p, 3, 2048u, __uint_as_float((uint32_t)(cm.lo ^ cm.hi)));
#if PSGPU_FIN_PHASES
        const uint64_t nvalid = (uint64_t)__popcll(ballot(s.valid));
        if ((p.debug & 2048u) && p.stamps && lane_id() == 0) {  // phase word 7: live primitives, vertices
            const uint32_t sw = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
            if (sw < p.stampCap)
                p.stamps[3 * (size_t)kNumStampKernels * p.stampCap + 8 * (size_t)sw + 7] =
                    (uint64_t)(128 - __popcll(cm.lo) - __popcll(cm.hi)) | (nvalid << 16);
        }
#endif
    }
    float g[4];  // the field at the four points
    if constexpr (VPW == 16) {
        const float qx = s.j == 1 ? P[0] + delta : P[0];
        const float qy = s.j == 2 ? P[1] + delta : P[1];
        const float qz = s.j == 3 ? P[2] + delta : P[2];
        float c4[3];
        const float f = ev.template eval<1, true>(qx, qy, qz, cm, c4);
        S.c[0] = quad_bcast<0>(c4[0]);
        S.c[1] = quad_bcast<0>(c4[1]);
        S.c[2] = quad_bcast<0>(c4[2]);
        quad_gather(f, g);
    } else if constexpr (VPW == 32) {
        // lane 0: P, P + delta e_x; lane 1: P + delta e_y, P + delta e_z
        const float qx[2] = {P[0], s.j == 0 ? P[0] + delta : P[0]};
        const float qy[2] = {s.j == 1 ? P[1] + delta : P[1], P[1]};
        const float qz[2] = {P[2], s.j == 1 ? P[2] + delta : P[2]};
        float f[2], c6[6];
        ev.template evaln<1, true, 2>(qx, qy, qz, cm, f, c6);
        const float o0 = PSGPU_DPP_F(f[0], 0xB1), o1 = PSGPU_DPP_F(f[1], 0xB1);
        const float oc0 = PSGPU_DPP_F(c6[0], 0xB1), oc1 = PSGPU_DPP_F(c6[1], 0xB1),
                    oc2 = PSGPU_DPP_F(c6[2], 0xB1);
        S.c[0] = s.j == 0 ? c6[0] : oc0;
        S.c[1] = s.j == 0 ? c6[1] : oc1;
        S.c[2] = s.j == 0 ? c6[2] : oc2;
        g[0] = s.j == 0 ? f[0] : o0;
        g[1] = s.j == 0 ? f[1] : o1;
        g[2] = s.j == 0 ? o0 : f[0];
        g[3] = s.j == 0 ? o1 : f[1];
    } else {
        const float qx[4] = {P[0], P[0] + delta, P[0], P[0]};
        const float qy[4] = {P[1], P[1], P[1] + delta, P[1]};
        const float qz[4] = {P[2], P[2], P[2], P[2] + delta};
        float c4[12];
        ev.template evaln<1, true, 4>(qx, qy, qz, cm, g, c4);
        if constexpr (STAMP) phase_stamp_after(p, 4, 2048u, g[0] + g[1] + g[2] + g[3] + c4[0] + c4[1] + c4[2]);
        S.c[0] = c4[0];
        S.c[1] = c4[1];
        S.c[2] = c4[2];
    }
    const float nx = (g[1] - g[0]) * inv;
    const float ny = (g[2] - g[0]) * inv;
    const float nz = (g[3] - g[0]) * inv;
    const float im = 1.0f / sqrtf((nx * nx + ny * ny) + nz * nz);
    S.n[0] = nx * im;
    S.n[1] = ny * im;
    S.n[2] = nz * im;
    return S;
}

// Stage: the vertex into the compact mesh at index gi.  Quad: lanes 0-2 write component j of
// position, normal and colour.  Pair: lane j writes component j, lane 0 also component 2.
// Wide: the lane writes all nine.  Past vCap nothing is written: finish() grows and re-runs.
// (values, not references into S: a choice between addresses would keep S in scratch memory)
__device__ __forceinline__ float component(int j, float x, float y, float z) { return j == 0 ? x : (j == 1 ? y : z); }
template <int VPW>
__device__ __forceinline__ void store_vertex(const Params& p, const VertexSlot& s, uint32_t gi, const float P[3],
                                             const Shaded& S) {
    if (!s.valid || gi >= p.vCap) return;
    if constexpr (VPW == 16) {
        if (s.j < 3) {
            const uint32_t o = gi * 3 + (uint32_t)s.j;
            p.pos[o] = component(s.j, P[0], P[1], P[2]);
            p.nrm[o] = component(s.j, S.n[0], S.n[1], S.n[2]);
            p.col[o] = component(s.j, S.c[0], S.c[1], S.c[2]);
        }
    } else if constexpr (VPW == 32) {
        const uint32_t o = gi * 3 + (uint32_t)s.j;
        p.pos[o] = s.j == 0 ? P[0] : P[1];
        p.nrm[o] = s.j == 0 ? S.n[0] : S.n[1];
        p.col[o] = s.j == 0 ? S.c[0] : S.c[1];
        if (s.j == 0) {
            p.pos[gi * 3 + 2] = P[2];
            p.nrm[gi * 3 + 2] = S.n[2];
            p.col[gi * 3 + 2] = S.c[2];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) p.pos[gi * 3 + c] = P[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) p.nrm[gi * 3 + c] = S.n[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) p.col[gi * 3 + c] = S.c[c];
    }
}

// k_surface's wait for the offsets scan (every scan block released its offsets), bounded: a
// broken protocol flags the run (error bit 1) instead of hanging the device.
// The flag reaches the host through words block 0 never overwrites (surfaceErr, raised with
// a plain store; totals[7], raised atomically), so a timeout after block 0 published the
// counters still fails the run, and psgpu_finish re-runs it as k_vertex + k_finish.
__device__ __forceinline__ void surface_wait_scan(const Params& p) {
    if (lane_id() == 0) {
        uint32_t spins = 0;
        // test hook (PSGPU_OPT_DEBUG bit 25): a bound far below the scan blocks' delay
        const uint32_t bound = (p.debug & (1u << 25)) ? 4u : (1u << 22);
        while (__hip_atomic_load(&p.ctr->scanDone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < p.scanBlocks) {
            __builtin_amdgcn_s_sleep(2);
            if (++spins > bound) {
                atomicOr(&p.ctr->error, 2u);
                atomicOr(&p.totals[7], 2u);
                p.hostCtr->surfaceErr = 2u;
                __threadfence_system();
                break;
            }
        }
    }
    // no agent-scope acquire here: on gfx950 it invalidates the XCD's L2 for every kernel on it
    // (measured: a 1/8 share 0.028 vs 0.015 ms/step).  The offsets are read with agent-scope
    // loads instead (surface_offs), which bypass the non-coherent caches and are issued only
    // after the flag was seen.
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
}
// an offsets word written by this launch's scan blocks (released before their scanDone count)
__device__ __forceinline__ uint64_t surface_offs(const Params& p, uint32_t i) {
    return __hip_atomic_load(&p.offs[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// An offsets word of either kernel: k_finish runs after the launch that scanned them and loads
// plainly; k_surface (FUSED) reads what its own scan blocks wrote.
template <bool FUSED>
__device__ __forceinline__ uint64_t offs_word(const Params& p, uint32_t i) {
    if constexpr (FUSED) return surface_offs(p, i);
    else return p.offs[i];
}

// Stage: block 0's duties at the end of a run.  The run's counters to the host (mapped pinned
// memory), then -- after a system fence, so the host never sees a reset it could mistake for
// this run's -- the next run's counters and offsets-scan words (no kernel of this run touches
// them), and the run's totals for the count exchange between parts (RCCL).
// FUSED (k_surface, called once every scan block is done): `error` is read at agent scope, so a
// look-back timeout of any scan block (error bit 0) is in what is published; the host's
// surfaceErr word is never overwritten and totals[7] is raised, never stored (k_precheck zeroed
// it), so a scan-wait timeout flagged by another wave after this survives (surface_wait_scan).
template <bool FUSED>
__device__ __forceinline__ void publish_run(const Params& p) {
    constexpr uint32_t kWords = sizeof(DevCounters) / 4;
    constexpr uint32_t kErrWord = __builtin_offsetof(DevCounters, error) / 4;
    constexpr uint32_t kSurfWord = __builtin_offsetof(DevCounters, surfaceErr) / 4;
    constexpr uint32_t kEpochWord = __builtin_offsetof(DevCounters, epoch) / 4;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(p.ctr);
    uint32_t* dst = reinterpret_cast<uint32_t*>(p.hostCtr);
    uint32_t err = 0u;  // FUSED: read once; the host's copy and totals[7] get this value
    if constexpr (FUSED) err = __hip_atomic_load(&p.ctr->error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t i = threadIdx.x; i < kWords; i += blockDim.x)
        if (!FUSED || i != kSurfWord) dst[i] = FUSED && i == kErrWord ? err : src[i];
    __threadfence_system();
    uint32_t* nx = reinterpret_cast<uint32_t*>(p.ctrNext);
    const uint32_t nextEpoch = p.ctr->epoch + 1u;
    for (uint32_t i = threadIdx.x; i < kWords; i += blockDim.x)
        nx[i] = i == 0 ? 0x7fffffffu : (i == kEpochWord ? nextEpoch : 0u);
    for (uint32_t i = threadIdx.x; i < kScanMaxBlocks; i += blockDim.x) p.scanStatusNext[i] = 0ull;
    if (threadIdx.x < 64) {
        const ShardCtr& sc = p.ctr->shard[threadIdx.x];
        const uint32_t tv = wave_sum(sc.v), tt = wave_sum(sc.t), tp = wave_sum(sc.p), tb = wave_sum(sc.b),
                       ts = wave_sum(sc.s);
        if (threadIdx.x == 0) {
            const uint32_t tot[8] = {p.mpuCount, tv, tt, tp + tb, ts, tp, (uint32_t)p.ctr->firstOverflow,
                                     FUSED ? err : p.ctr->error};
            for (int i = 0; i < (FUSED ? 7 : 8); ++i) p.totals[i] = tot[i];
            if (FUSED && err) atomicOr(&p.totals[7], err);
        }
    }
}

// Stage: triangle records -> global vertex ids.  A record holds three 11-bit MPU-local vertex
// ids and its local triangle id; its MPU's offsets word gives the bases of both.  Past tCap
// nothing is written: finish() grows and re-runs.
template <bool FUSED>
__device__ __forceinline__ void triangle_pass(const Params& p, const ShardBatches& sb, uint32_t wave0,
                                              uint32_t nWaves) {
    for (uint32_t batch = wave0; batch < sb.total; batch += nWaves) {
        uint32_t shard, first, count;
        sb.locate(batch, &shard, &first, &count);
        const uint32_t t = first + lane_id();
        if (t >= count) continue;
        const TriRec R = p.tq[(size_t)shard * p.tShardCap + t];
        const uint64_t o = offs_word<FUSED>(p, ((R.a >> 12) << 6) | shard);  // the record's shard is w & 63
        const uint32_t gt = (uint32_t)(o >> 32) + (R.a & 2047u);
        const uint32_t base = (uint32_t)o;
        if (gt >= p.tCap) continue;
        p.tris[gt * 3 + 0] = base + (R.b & 2047u);
        p.tris[gt * 3 + 1] = base + ((R.b >> 11) & 2047u);
        p.tris[gt * 3 + 2] = base + ((R.b >> 22) | (((R.a >> 11) & 1u) << 10));
    }
}

// k_vertex: the first blocks scan the offsets (scan_counts_block); every wave then brackets
// the roots of its batches of vertex records, quad or wide, and stores bracket and scale into
// the record.  k_finish recomputes the position from them (vertex_root).
template <class EV, int VPW = 16>
__device__ __forceinline__ void vertex_body(const Params& p, float* lds) {
    const int wave = wave_index();
    EV ev(as_const(p.model), lds + wave * (p.slotsPerLane * 4 * 64) + lane_id());
    if (blockIdx.x < p.scanBlocks) scan_counts_block(p, blockIdx.x);  // block-uniform
    __shared__ uint32_t sCnt[kShards];
    stage_shard_counts(p, 1, sCnt);  // ShardCtr::v
    __syncthreads();
    const uint32_t nWaves = gridDim.x * (blockDim.x >> 6);
    const ShardBatches sb(sCnt, p.vShardCap, VPW);
    for (uint32_t batch = blockIdx.x * (blockDim.x >> 6) + wave; batch < sb.total; batch += nWaves) {
        const VertexSlot s = locate_vertex<VPW>(p, sb, batch);
        const VertexKey K = p.vk[s.rec];
        const VertexPos R =
            root_bracket<EV, VPW>(ev, p, edge_segment(p, K.w, K.vidKey >> 16), edge_mask(p, K.w), s);
        if (s.valid && s.j == 0) p.vp[s.rec] = R;
    }
}

// k_finish, after k_vertex wrote the roots: block 0 publishes the run; every wave then shades
// the vertices of its batches of records (wide, quad or pair) into the mesh, then resolves its
// batches of triangle records.
// PSGPU_FIN_PHASES stamps the wide loop only: 2 = records in and root recomputed, 3-4 inside
// shade_vertex, 5 = stored.
template <class EV, int VPW = 64>
__device__ __forceinline__ void finish_body(const Params& p, float* lds) {
    constexpr bool kStamp = VPW == 64;
    const int wave = wave_index();
    EV ev(as_const(p.model), lds + wave * (p.slotsPerLane * 4 * 64) + lane_id());
    const uint32_t nWaves = gridDim.x * (blockDim.x >> 6);
    const uint32_t wave0 = blockIdx.x * (blockDim.x >> 6) + wave;
    phase_stamp_after(p, 0, 2048u, 0.0f);
    if (blockIdx.x == 0) publish_run<false>(p);
    __shared__ uint32_t sCnt[2 * kShards];
    stage_shard_counts(p, 1, sCnt);            // ShardCtr::v
    stage_shard_counts(p, 2, sCnt + kShards);  // ShardCtr::t
    __syncthreads();
    phase_stamp_after(p, 1, 2048u, 0.0f);
    const ShardBatches sv(sCnt, p.vShardCap, VPW);
    for (uint32_t batch = wave0; batch < sv.total; batch += nWaves) {
        const VertexSlot s = locate_vertex<VPW>(p, sv, batch);
        const VertexKey K = p.vk[s.rec];
        const VertexPos R = p.vp[s.rec];
        const uint32_t gi = (uint32_t)offs_word<false>(p, K.w) + (K.vidKey & 0xffffu);
        float P[3];
        vertex_root(edge_segment(p, K.w, K.vidKey >> 16), R.iv, R.scale, P);
        if constexpr (kStamp) phase_stamp_after(p, 2, 2048u, P[0] + P[1] + P[2]);
        const Shaded S = shade_vertex<EV, VPW, kStamp>(ev, p, P, R.scale >= 0.0f && R.scale <= 1.0f, s,
                                                       [&] { return cull_mask_mpus(p, K.w); });
        store_vertex<VPW>(p, s, gi, P, S);
        if constexpr (kStamp) phase_stamp_after(p, 5, 2048u, __uint_as_float(gi));
    }
    if (p.debug & 64u) return;  // ablation bit 6: no triangles
    triangle_pass<false>(p, ShardBatches(sCnt + kShards, p.tShardCap, 64), wave0, nWaves);
    phase_stamp_after(p, 6, 2048u, 0.0f);
}

// k_front (PSGPU_OPT_FRONT): k_precheck and k_mpu as one launch for small launches, with a
// dataflow hand-over instead of the kernel boundary (no grid barrier: r05's barrier version,
// k_front v1-v3 in profiles/r05_front_ab.txt, was slower than the boundary).  Blocks
// [0, preBlocks) run S1 exactly as k_precheck and publish each queued MPU (sc1 entry and
// culling mask, then the entry's ready word with the run's tag) into sub-queue blockIdx & 7;
// when all of a block's waves have published, its last wave counts the block done for its
// sub-queue.  The blocks after them run S2-S3 exactly as k_mpu on entries as they are
// published.  Every S1 block is dispatched before any S2 block (in-order dispatch), so a
// waiting S2 block never holds back the S1 block it waits for; every wait is bounded and a
// timeout fails the run as a protocol error (finish re-runs it as separate launches).
template <class EV, int SPLIT>
__device__ __forceinline__ void front_body(const Params& p, unsigned char* smem) {
    const uint64_t t0 = (p.stamps || p.spans) ? stamp_now() : 0ull;
    if (blockIdx.x < p.preBlocks) {  // block-uniform
        __shared__ uint32_t sArrive;
        if (threadIdx.x == 0) {
            sArrive = 0u;
            if (p.debug & (1u << 27)) {  // test hook: the S1 blocks publish ~40 us late
                const uint64_t h0 = stamp_now();
                while (stamp_now() - h0 < 4000u) __builtin_amdgcn_s_sleep(8);
            }
        }
        __syncthreads();
        precheck_body<EV, SPLIT, true>(p, reinterpret_cast<float*>(smem));
        if (p.stamps) stamp_end(p, 0, t0, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
        if (p.spans) span_end(p, 0, t0);
        // the block's arrival: each wave after its own stores left it; the last one signals
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane_id() == 0 && atomicAdd(&sArrive, 1u) == (blockDim.x >> 6) - 1u)
            __hip_atomic_fetch_add(&p.ctr->shard[blockIdx.x & 7u].s1Done, 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    } else {
        const uint32_t blk = blockIdx.x - p.preBlocks;
        uint32_t item = 0xffffffffu;
        mpu_body<EV, SPLIT, true>(p, smem, &item, blk);
        if (p.stamps) stamp_end(p, 1, t0, item, blk);
        if (p.spans) span_end(p, 1, t0);
    }
}

// k_surface (PSGPU_OPT_FUSED_SURFACE): k_vertex and k_finish in one launch for small launches
// (a rank's share; the launch floor, not the work, sets their step: DESIGN.md §5), quad layout;
// k_surface_w (PSGPU_OPT_FUSED_SURFACE 3, VPW 64): the wide layout, for launches whose vertices
// fill the device.  Per vertex the stages of both kernels in one loop, with the root's bracket
// and scale kept in registers instead of the vertex record, and the bracket's MPU masks reused
// for the shading.  The first blocks run the offsets scan as in k_vertex and release it; block 0
// publishes the run once every scan block is done; any other wave waits for the scan only before
// its first mesh write.  The scan blocks have the lowest block ids, so they are dispatched before
// any waiting block of their XCD: the wait cannot starve them.
template <class EV, int VPW = 16>
__device__ __forceinline__ void surface_body(const Params& p, float* lds) {
    const int wave = wave_index();
    EV ev(as_const(p.model), lds + wave * (p.slotsPerLane * 4 * 64) + lane_id());
    const uint32_t nWaves = gridDim.x * (blockDim.x >> 6);
    const uint32_t wave0 = blockIdx.x * (blockDim.x >> 6) + wave;
    if (blockIdx.x < p.scanBlocks) {  // block-uniform
        scan_counts_block(p, blockIdx.x);
        __syncthreads();  // the block's offsets stores are in L2
        if (threadIdx.x == 0) {
            if (p.debug & (1u << 25)) {  // test hook: the scan blocks count themselves done ~40 us late
                const uint64_t t0 = stamp_now();
                while (stamp_now() - t0 < 4000u) __builtin_amdgcn_s_sleep(8);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // ... and written back for the other XCDs
            __hip_atomic_fetch_add(&p.ctr->scanDone, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < 64) surface_wait_scan(p);
        __syncthreads();
        publish_run<true>(p);
    }
    __shared__ uint32_t sCnt[2 * kShards];
    stage_shard_counts(p, 1, sCnt);            // ShardCtr::v
    stage_shard_counts(p, 2, sCnt + kShards);  // ShardCtr::t
    __syncthreads();
    bool scanSeen = blockIdx.x == 0;  // block 0 waited above
    const ShardBatches sv(sCnt, p.vShardCap, VPW);
    for (uint32_t batch = wave0; batch < sv.total; batch += nWaves) {
        const VertexSlot s = locate_vertex<VPW>(p, sv, batch);
        const VertexKey K = p.vk[s.rec];
        const EdgeSeg E = edge_segment(p, K.w, K.vidKey >> 16);
        const CullMask cmv = edge_mask(p, K.w);
        const VertexPos R = root_bracket<EV, VPW>(ev, p, E, cmv, s);
        float P[3];
        vertex_root(E, R.iv, R.scale, P);
        const Shaded S =
            shade_vertex<EV, VPW>(ev, p, P, R.scale >= 0.0f && R.scale <= 1.0f, s, [&] { return cmv; });
        if (!scanSeen) {
            surface_wait_scan(p);
            scanSeen = true;
        }
        const uint32_t gi = (uint32_t)offs_word<true>(p, K.w) + (K.vidKey & 0xffffu);
        store_vertex<VPW>(p, s, gi, P, S);
    }
    if (p.debug & 64u) return;  // ablation bit 6: no triangles
    const ShardBatches st(sCnt + kShards, p.tShardCap, 64);
    if (wave0 < st.total && !scanSeen) surface_wait_scan(p);
    triangle_pass<true>(p, st, wave0, nWaves);
}

// Field probe for tests: mode 0 quads of consecutive points, 1 per point, 2 + colour.
template <class EV>
__device__ __forceinline__ void probe_body(const Params& p, float* lds, const float* xyz, float* out, float* colOut,
                                           uint32_t n, int mode) {
    const int wave = wave_index();
    ModelPtr M = as_const(p.model);
    EV ev(M, lds + wave * (p.slotsPerLane * 4 * 64) + lane_id());
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n;
    if (!valid) i = (n ? n - 1 : 0);
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    const CullMask cm = cull_mask_points(M, x, y, z, p.cull != 0);
    float c[3] = {0.0f, 0.0f, 0.0f};
    float f;
    if (mode == 0) f = ev.template eval<4, false>(x, y, z, cm, nullptr);
    else if (mode == 1) f = ev.template eval<1, false>(x, y, z, cm, nullptr);
    else f = ev.template eval<1, true>(x, y, z, cm, c);
    if (valid) {
        out[i] = f;
        if (colOut) {
            colOut[3 * i] = c[0];
            colOut[3 * i + 1] = c[1];
            colOut[3 * i + 2] = c[2];
        }
    }
}

}  // namespace psgpu
