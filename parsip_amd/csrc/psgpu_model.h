// psgpu_model.h — device-side image of a linearised BlobTree (host + device).
//
// The reference walks the op tree per SIMD call with an explicit stack
// (FieldComputer::fieldValue, PS_Polygonizer.cpp:1184-1376).  On CDNA4 every
// wavefront walks the same tree, so the host flattens the walk once per model into
// a short wave-uniform program (read with scalar loads) and the per-lane state is
// reduced to a resume pc (op-box pruning) plus a small value stack in LDS.
//
//   ENTER  op, skipTo, out   depth>3 op-box test (PS_Polygonizer.cpp:1228-1252);
//                            lanes whose 4-lane group is outside resume at skipTo
//                            with field 0 in slot `out`.
//   PRIM   prim, out         computePrimitiveField (:934-1179) into slot `out`.
//   OP     op, type, l, r    binary combine (:1282-1338) into slot `out`.
//   SUMPRIM prim             no-op trees: running sum of all prims (:1356-1368).
//
// The program order is the reference's processing order (post-order, right child
// first, :1344-1352), which also fixes the "stale outField" semantics of op types
// that have no case in the reference switch.
#pragma once
#ifdef __HIPCC_RTC__
// hiprtc (run-time specialised kernels, psgpu_jit.cpp): no system headers
typedef unsigned char uint8_t;
typedef signed char int8_t;
typedef unsigned short uint16_t;
typedef unsigned int uint32_t;
typedef int int32_t;
typedef unsigned long long uint64_t;
typedef long long int64_t;
#elif defined(PSGPU_MODEL_NO_HIP)
#include <stdint.h>  // a plain C++ host program (tests/cpp/op_inside_check.cpp)
#include <string.h>
#include <mutex>
#include <vector>
#else
#include <stdint.h>
#include <string.h>
#include <hip/hip_runtime.h>
#include <mutex>
#include <vector>
#endif
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define PSGPU_HD __host__ __device__
#define PSGPU_HDI __host__ __device__ __forceinline__  // inlined into the kernels: no call, no call ABI's registers
#else
#define PSGPU_HD
#define PSGPU_HDI inline
#endif

namespace psgpu {

// "Op-inside" predicate (k_precheck makes one bit per op and queued MPU from it; the walks skip
// the op-box pruning test of an op whose bit is set: Gen::emit_op, psgpu_jit.cpp).  The pruning
// test of a point q is in(q) = OR over the axes of (q >= lo && hi >= q) (PS_Polygonizer.cpp:
// 1228-1252), so it cannot prune anything when, along one axis, every coordinate a walk can see
// under the MPU lies in the op's [lo, hi].  True when the MPU's extent [o, o + 7 cs] along the
// axis, grown on both sides by m = 0.002 + 1e-5 * max(|o|, |o + 7 cs|), lies in [lo, hi] (the
// walk's own fp32 compares; NaN compares false, and a box of magnitude >= 1e30 sets no bit).
//
// Why m suffices.  Write M = max(|o|, |o + 7 cs|) and u = 2^-24 (fp32 half-ulp, relative).  The
// coordinates walked under an MPU, along one axis, are
//   S2 corners       fl(o + fl(x cs)), x = 0..7                                  (mpu_body)
//   edge samples     e = fl(o + fl(cs s)), s <= 7;  d = fl(fl(e + cs) - e) where the edge runs
//                    along this axis (then s <= 6), else 0;  fl(e + fl(d t)), t in [0, 1]
//                                                                  (edge_segment, edge_sample)
//   roots            fl(a + fl(scale fl(b - a))), a, b two edge samples, scale in [0, 1]: k_finish
//                    takes the MPU masks only when every vertex of the wave is on its segment
//   normal points    fl(root + 0.001f)                                          (shade_vertex)
// In exact arithmetic the first three lie in [o, o + 7 cs] and the last within 0.001f <
// 0.0010001 of it.  Every fl() above rounds a value of magnitude <= M + 0.0011 (or a product
// below it), so it moves the result by at most u (M + 0.0011); a coordinate depends on at most
// 12 of them (both samples of a root counted), so it lies within 0.0010001 + 12 u (M + 0.0011)
// < 0.00101 + 7.2e-7 M of the exact extent.  The grown box is computed with 5 roundings of its own (7 cs, o + 7 cs, 1e-5 M, m,
// the final o - m or hi + m), each below u (M + m): it shrinks by less than 3.1e-7 (M + m), so
// it still reaches 0.0019 + 0.9e-5 M past the exact extent, which covers the coordinates'
// 0.00101 + 7.2e-7 M for every finite M.  No culling slack is involved.
PSGPU_HD inline bool op_inside_axis(float opLo, float opHi, float o, float cs) {
    const float hi = o + 7.0f * cs;
    const float mag = __builtin_fmaxf(__builtin_fabsf(o), __builtin_fabsf(hi));
    if (!(mag < 1e30f)) return false;
    const float m = 0.002f + 1e-5f * mag;
    return opLo <= o - m && hi + m <= opHi;
}
PSGPU_HD inline bool op_inside_box(const float opLo[3], const float opHi[3], float ox, float oy, float oz, float cs) {
    return op_inside_axis(opLo[0], opHi[0], ox, cs) || op_inside_axis(opLo[1], opHi[1], oy, cs) ||
           op_inside_axis(opLo[2], opHi[2], oz, cs);
}

// Node type codes of the hot path (PS_Polygonizer.h:84-91; same as PsNodeType).
#define PSGPU_T_CYLINDER 0
#define PSGPU_T_DISC 1
#define PSGPU_T_LINE 2
#define PSGPU_T_POINT 3
#define PSGPU_T_RING 4
#define PSGPU_T_CUBE 6
#define PSGPU_T_TRIANGLE 7
#define PSGPU_T_UNION 14
#define PSGPU_T_INTERSECT 15
#define PSGPU_T_DIF 16
#define PSGPU_T_SMOOTHDIF 17
#define PSGPU_T_BLEND 18
#define PSGPU_T_RICCI 19

// Marching-cubes tables in device memory (generated on the host: cube_tables and
// fill_device_tables below), packed so a cell's whole row is one 64-bit word (4 bits per edge id):
//   row[c]   the triangle row g_triTableCache[c] (<= 15 entries)
//   order[c] the row's distinct edges in first-occurrence order (<= 12)
//   cross[c] 12-bit mask of sign-changing edges (== the row's edge set)
//   ntri[c]  triangles in the row
//   own[b]   12-bit mask of edges a cell owns, b = (i==0)<<2 | (j==0)<<1 | (k==0)
//   edge     per edge: corner1 (3 bits) | axis << 3, 5 bits per edge
//   crossNtri[c] cross[c] | ntri[c] << 16 (pass 1's one lookup per cell)
// k_mpu reads them from global memory (the 5.9 KB stay in every CU's L1 / L2).
struct CubeTablesDev {
    uint64_t row[256];
    uint64_t order[256];
    uint16_t cross[256];
    uint8_t ntri[256];
    uint16_t own[8];
    uint64_t edge;
    uint8_t pad[8];
    uint32_t crossNtri[256];
};

#ifndef __HIPCC_RTC__
// Marching-cubes table.  Generated, not transcribed: Bloomenthal's cube-table
// construction ("An Implicit Surface Polygonizer", Graphics Gems IV, 1994) walks
// each sign-changing edge clockwise around the cube faces to build polygons; the
// reference's g_triTableCache (_CellConfigTable.h:60-317) keeps polygons in
// discovery order with each polygon's edges in reverse walk order and fans
// triangles about the last edge.  Corner c: bit2 = x, bit1 = y, bit0 = z.
struct CubeTables {
    int8_t tri[256][16];
    uint8_t ntri[256];
    uint8_t corner1[12], corner2[12], axis[12];
};

inline const CubeTables& cube_tables() {
    static CubeTables T;
    static std::once_flag once;
    std::call_once(once, [] {
        // edges LB LT LN LF RB RT RN RF BN BF TN TF; faces L R B T N F
        static const uint8_t c1[12] = {0, 2, 0, 1, 4, 6, 4, 5, 0, 1, 2, 3};
        static const uint8_t c2[12] = {1, 3, 2, 3, 5, 7, 6, 7, 4, 5, 6, 7};
        static const uint8_t ax[12] = {2, 2, 1, 1, 2, 2, 1, 1, 0, 0, 0, 0};
        static const uint8_t lface[12] = {2, 0, 0, 5, 1, 3, 4, 1, 4, 2, 3, 5};
        static const uint8_t rface[12] = {0, 3, 4, 0, 2, 1, 1, 5, 2, 5, 4, 3};
        // next clockwise edge around `face` after `edge`: {face of the edge's first
        // listed face, next-if-that-face, next-otherwise}
        static const uint8_t ccwFace[12] = {0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3};
        static const uint8_t nextOn[12] = {3, 2, 0, 1, 6, 7, 5, 4, 4, 0, 1, 5};
        static const uint8_t nextOff[12] = {8, 11, 10, 9, 9, 10, 8, 11, 2, 7, 6, 3};
        memcpy(T.corner1, c1, 12);
        memcpy(T.corner2, c2, 12);
        memcpy(T.axis, ax, 12);
        for (int cfg = 0; cfg < 256; ++cfg) {
            auto in = [cfg](int c) { return (cfg >> c) & 1; };
            bool done[12] = {};
            std::vector<int> rows;
            for (int e = 0; e < 12; ++e) {
                if (done[e] || in(c1[e]) == in(c2[e])) continue;
                std::vector<int> poly;
                int edge = e, face = in(c1[e]) ? rface[e] : lface[e];
                for (;;) {
                    edge = (face == ccwFace[edge]) ? nextOn[edge] : nextOff[edge];
                    done[edge] = true;
                    if (in(c1[edge]) != in(c2[edge])) {
                        poly.insert(poly.begin(), edge);
                        if (edge == e) break;
                        face = (face == lface[edge]) ? rface[edge] : lface[edge];
                    }
                }
                const int np = (int)poly.size();
                for (int t = np - 3; t >= 0; --t) {
                    rows.push_back(poly[t]);
                    rows.push_back(poly[t + 1]);
                    rows.push_back(poly[np - 1]);
                }
            }
            for (int i = 0; i < 16; ++i) T.tri[cfg][i] = i < (int)rows.size() ? (int8_t)rows[i] : (int8_t)-1;
            T.ntri[cfg] = (uint8_t)(rows.size() / 3);
        }
    });
    return T;
}

// Packed device tables (CubeTablesDev above).
inline void fill_device_tables(const CubeTables& T, CubeTablesDev& D) {
    memset(&D, 0, sizeof(D));
    for (int c = 0; c < 256; ++c) {
        uint64_t row = 0, order = 0;
        uint32_t seen = 0;
        int nd = 0;
        for (int e = 0; e < 16 && T.tri[c][e] >= 0; ++e) {
            const int ed = T.tri[c][e];
            row |= (uint64_t)ed << (4 * e);
            if (!((seen >> ed) & 1u)) {
                seen |= 1u << ed;
                order |= (uint64_t)ed << (4 * nd++);
            }
        }
        uint32_t cross = 0;
        for (int e = 0; e < 12; ++e)
            if (((c >> T.corner1[e]) & 1) != ((c >> T.corner2[e]) & 1)) cross |= 1u << e;
        D.row[c] = row;
        D.order[c] = order;
        D.cross[c] = (uint16_t)cross;
        D.ntri[c] = T.ntri[c];
        D.crossNtri[c] = cross | ((uint32_t)T.ntri[c] << 16);
    }
    // ownership: the first cell in (i,j,k) order containing an edge owns it; an edge
    // starting at cell corner (cx,cy,cz) on axis a is owned by this cell iff every
    // non-axis corner bit is 1 or the cell sits on that axis' low boundary
    for (int b = 0; b < 8; ++b) {
        const bool i0 = b & 4, j0 = b & 2, k0 = b & 1;
        uint32_t m = 0;
        for (int e = 0; e < 12; ++e) {
            const int c1 = T.corner1[e], ax = T.axis[e];
            const bool bx = (c1 >> 2) & 1, by = (c1 >> 1) & 1, bz = c1 & 1;
            const bool okx = ax == 0 || bx || i0, oky = ax == 1 || by || j0, okz = ax == 2 || bz || k0;
            if (okx && oky && okz) m |= 1u << e;
        }
        D.own[b] = (uint16_t)m;
    }
    uint64_t edge = 0;
    for (int e = 0; e < 12; ++e) edge |= (uint64_t)(T.corner1[e] | (T.axis[e] << 3)) << (5 * e);
    D.edge = edge;
}
#endif  // !__HIPCC_RTC__

enum InstrKind : uint8_t { kEnter = 0, kPrim = 1, kOp = 2, kSumPrim = 3 };

struct Instr {           // 16 B, one s_load_dwordx4
    uint8_t kind;
    uint8_t type;        // OP: op type (PS_Polygonizer.h enum)
    uint8_t out;         // value slot written
    uint8_t lslot;       // OP: slot of left child value
    uint8_t rslot;       // OP: slot of right child value
    uint8_t childKind;   // OP: bit1 left is op, bit0 right is op
    uint8_t L, R;        // OP: child indices (prim or op ids)
    uint16_t idx;        // ENTER/OP: op id; PRIM/SUMPRIM: prim id
    uint16_t skipTo;     // ENTER: pc after the op's OP instruction
    uint32_t pad;
};
static_assert(sizeof(Instr) == 16, "Instr size");

struct DevOp {           // 32 B
    float lo[3];
    float hi[3];
    float resY;          // RicciBlend exponent (SOABlobOps::resY)
    uint32_t type;
};
static_assert(sizeof(DevOp) == 32, "DevOp size");

struct DevPrim {         // 128 B
    float pos[3];
    float dir[3];
    float res[3];
    float col[3];
    uint32_t type;
    uint32_t hasMatrix;  // idxMatrix != 0
    uint32_t cullable;   // bit 0: exact culling bound valid; 1: unbounded line; 2: axis clearance
    float cullRadius;    // skeleton-to-surface slack of the bound (cube: half diagonal)
    float mat[12];       // SOABlobPrimMatrices row-major 3x4 (12-float stride)
    float pad[4];
};
static_assert(sizeof(DevPrim) == 128, "DevPrim size");

constexpr int kMaxInstr = 512;
constexpr int kMaxSlots = 64;

// Culling skeleton of a primitive: the segment A + t*U, t in [tmin, tmax] ([0,1]; any t
// for the unbounded Line), whose distance minus `radius` bounds the primitive's distance
// from below; one branch-free formula for every slot: radius = +inf never culls (not
// eligible, or past ctPrims), -inf always culls (Triangle: field exactly 0).
struct CullSeg {         // 48 B: three 16-B loads per lane
    float a[3];
    float u[3];
    float invUU;         // 1 / |U|^2, 0 for a point
    float radius;
    float tmin, tmax;
    float axisClear;     // the box must keep this distance from the segment's line (Cylinder: its
                         // rounded-negative sqrt is NaN on the axis); -inf: no condition
    float boxHalf;       // the primitive is the axis-aligned box of this half side round A (Point: 0,
                         // Cube: its half side), which the gap form of cull_one uses; +inf: it is not
                         // one (Line, Cylinder, every slot that is never culled) and the form gives 0
};
static_assert(sizeof(CullSeg) == 48, "CullSeg size");

// sqrt of the culling tests: the device's v_sqrt_f32, the host's sqrtf (a plain C++ program
// compiles these tests too: tests/cpp/sieve_check.cpp)
PSGPU_HDI float cull_sqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(x);
#else
    return __builtin_sqrtf(x);
#endif
}

// Centre c and half-diagonal h (grown by its rounding) of the box [x0, x1] x [y0, y1] x [z0, z1]
// for cull_one; false for a box that is not finite (a NaN compares false): nothing is culled.
PSGPU_HDI bool cull_box(float x0, float y0, float z0, float x1, float y1, float z1, float c[3], float* h) {
    if (!(x1 - x0 < 1e30f && y1 - y0 < 1e30f && z1 - z0 < 1e30f)) return false;
    c[0] = 0.5f * (x0 + x1);
    c[1] = 0.5f * (y0 + y1);
    c[2] = 0.5f * (z0 + z1);
    const float hx = 0.5f * (x1 - x0), hy = 0.5f * (y1 - y0), hz = 0.5f * (z1 - z0);
    *h = cull_sqrt(hx * hx + hy * hy + hz * hz) * 1.0001f + 1e-6f;
    return true;
}

// Half-extent of [x0, x1] about the centre c as computed (0.5f * (x0 + x1), rounded: off the true
// centre by at most half an ulp of c, 2^-24 |c|, which the last term covers twice over).
PSGPU_HDI float box_half_extent(float x0, float x1, float c) { return 0.5f * (x1 - x0) + __builtin_fabsf(1.2e-7f * c); }

// The same, and the box's half-extents e along x, y, z, each grown by its rounding as h is.
PSGPU_HDI bool cull_box(float x0, float y0, float z0, float x1, float y1, float z1, float c[3], float* h,
                        float e[3]) {
    if (!cull_box(x0, y0, z0, x1, y1, z1, c, h)) return false;
    e[0] = box_half_extent(x0, x1, c[0]) * 1.0001f + 1e-6f;
    e[1] = box_half_extent(y0, y1, c[1]) * 1.0001f + 1e-6f;
    e[2] = box_half_extent(z0, z1, c[2]) * 1.0001f + 1e-6f;
    return true;
}

// 1 / x for the box bounds: the device's v_rcp_f32 (1 ulp, inside the bounds' relative 1e-4)
PSGPU_HDI float cull_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}

// Is the segment's primitive exactly +0 over the box (centre c, half-diagonal h)?  The box as its
// circumscribed sphere: the distance d to the skeleton is 1-Lipschitz, so d(q) >= d(c) - h at
// every point q of the box.  (k_sieve's form, which tests/cpp/sieve_check.cpp compiles.)
PSGPU_HDI bool cull_one(const CullSeg& S, float cx, float cy, float cz, float h) {
    const float dx = cx - S.a[0], dy = cy - S.a[1], dz = cz - S.a[2];
    const float t = (dx * S.u[0] + dy * S.u[1] + dz * S.u[2]) * S.invUU;
    const float lx = dx - t * S.u[0], ly = dy - t * S.u[1], lz = dz - t * S.u[2];
    const float lineDist = cull_sqrt(lx * lx + ly * ly + lz * lz);
    const float tc = __builtin_fminf(__builtin_fmaxf(t, S.tmin), S.tmax);
    const float ex = dx - tc * S.u[0], ey = dy - tc * S.u[1], ez = dz - tc * S.u[2];
    const float d = (cull_sqrt(ex * ex + ey * ey + ez * ez) - S.radius) - h;
    return d > 0.0f && d * d >= 1.02f && (lineDist - h > S.axisClear);
}

// The same question with the box as the box it is (half-extents he, from cull_box).  A skeleton
// K (a point, a line, a segment) is a convex set, and so is an axis-aligned cube.  Let p* be the
// point of K nearest the box centre c and e = c - p*.  K lies in the half-space
// <x - p*, e> <= 0 (the projection inequality), so for q = c + w in the box
//   support form   d(q) >= <q - p*, e> / |e| = |e| + <w, e> / |e|
//                       >= |e| - (he_x |e_x| + he_y |e_y| + he_z |e_z|) / |e|,
// which by Cauchy-Schwarz is never below the sphere's |e| - h: a box whose face is turned
// towards K pays its half-side, not its half-diagonal.  Where the primitive is itself an
// axis-aligned box of half side s round A (Point: s = 0; Cube) the distance between the two
// boxes is exact:
//   gap form       d(q) >= sqrt(sum_a max(0, |c_a - A_a| - he_a - s)^2),
// and it replaces the cube's ball of radius s sqrt(3).  The bound is the maximum of the three,
// so it culls whatever the sphere form culls.  Every new term is rounded against culling (the
// half-extents and the support term grow by a relative 1e-4 and 1e-6); |e| = 0 or a non-finite
// term gives NaN or -inf, which the maximum drops.  The acceptance d > 0, d^2 >= 1.02 and the
// axis clearance are the sphere form's.
PSGPU_HDI bool cull_one(const CullSeg& S, float cx, float cy, float cz, float h, const float he[3]) {
    const float dx = cx - S.a[0], dy = cy - S.a[1], dz = cz - S.a[2];
    const float t = (dx * S.u[0] + dy * S.u[1] + dz * S.u[2]) * S.invUU;
    const float lx = dx - t * S.u[0], ly = dy - t * S.u[1], lz = dz - t * S.u[2];
    const float lineDist = cull_sqrt(lx * lx + ly * ly + lz * lz);
    const float tc = __builtin_fminf(__builtin_fmaxf(t, S.tmin), S.tmax);
    const float ex = dx - tc * S.u[0], ey = dy - tc * S.u[1], ez = dz - tc * S.u[2];
    const float n = cull_sqrt(ex * ex + ey * ey + ez * ez);
    const float sphere = (n - S.radius) - h;
    const float reach = (he[0] * __builtin_fabsf(ex) + he[1] * __builtin_fabsf(ey) + he[2] * __builtin_fabsf(ez)) *
                        cull_rcp(n);
    const float support = (n - S.radius) - (reach * 1.0001f + 1e-6f);
    const float gx = __builtin_fmaxf((__builtin_fabsf(dx) - he[0]) - S.boxHalf, 0.0f);
    const float gy = __builtin_fmaxf((__builtin_fabsf(dy) - he[1]) - S.boxHalf, 0.0f);
    const float gz = __builtin_fmaxf((__builtin_fabsf(dz) - he[2]) - S.boxHalf, 0.0f);
    const float gap = cull_sqrt(gx * gx + gy * gy + gz * gz);
    const float d = __builtin_fmaxf(__builtin_fmaxf(sphere, support), gap);  // fmaxf drops a NaN
    return d > 0.0f && d * d >= 1.02f && (lineDist - h > S.axisClear);
}

// Field interval of one primitive over a box (the field bounds of k_precheck: see prim_bound,
// psgpu_device.h, which explains what the interval proves).  Point, infinite Line, solid capped
// Cylinder and axis-aligned Cube are convex sets K, and the functions below are their true
// Euclidean distances.  With p* the point of K nearest the box centre c, e = c - p* and d = |e|,
// every point q = c + w of the box (half-extents hx, hy, hz; half-diagonal h) has
//   d(q) >= d - h                                        (1-Lipschitz)
//   d(q) >= d - (hx |e_x| + hy |e_y| + hz |e_z|) / d     (support form, see cull_one; >= d - h)
//   d(q) >= sqrt(sum_a max(0, |e_a| - h_a)^2)            (Point, Cube: the boxes' exact gap)
//   d(q) <= |q - p*| <= sqrt(sum_a (|e_a| + h_a)^2)      (<= d + h by the triangle inequality)
// and Wyvill's field is monotone in the distance.  h and the half-extents come with their slack
// (octant_box: a relative 1e-4 and 1e-4, which every term above inherits), and the field
// interval is widened by kBoundEps, orders of magnitude above the fp32 rounding of either
// evaluation (where d > 2 that rounding may exceed the slack, and the field is 0 at either
// end).  d = 0 makes the support term NaN, which fmaxf drops.
constexpr float kBoundEps = 2e-4f;

// Distance of (x, y, z) from the primitive; ev = |e_a|; axisD: a Cylinder's distance from its axis.
template <int TYPE, class PR>
PSGPU_HDI float prim_true_dist(PR& P, float x, float y, float z, float* axisD, float ev[3]) {
    float d2 = 0.0f;
    ev[0] = ev[1] = ev[2] = 0.0f;
    if (TYPE == PSGPU_T_POINT) {
        const float dx = x - P.pos[0], dy = y - P.pos[1], dz = z - P.pos[2];
        ev[0] = __builtin_fabsf(dx); ev[1] = __builtin_fabsf(dy); ev[2] = __builtin_fabsf(dz);
        d2 = dx * dx + dy * dy + dz * dz;
    } else if (TYPE == PSGPU_T_LINE) {  // distance from the infinite line (the reference does not clamp)
        const float ux = P.dir[0] - P.pos[0], uy = P.dir[1] - P.pos[1], uz = P.dir[2] - P.pos[2];
        const float dx = x - P.pos[0], dy = y - P.pos[1], dz = z - P.pos[2];
        const float t = (dx * ux + dy * uy + dz * uz) / (ux * ux + uy * uy + uz * uz);
        const float ex = dx - t * ux, ey = dy - t * uy, ez = dz - t * uz;
        ev[0] = __builtin_fabsf(ex); ev[1] = __builtin_fabsf(ey); ev[2] = __builtin_fabsf(ez);
        d2 = ex * ex + ey * ey + ez * ez;
    } else if (TYPE == PSGPU_T_CYLINDER) {  // solid cylinder: axis dir (unit), radius res0, height res1
        const float px = x - P.pos[0], py = y - P.pos[1], pz = z - P.pos[2];
        float yy = px * P.dir[0] + py * P.dir[1] + pz * P.dir[2];
        const float rr = px * px + py * py + pz * pz - yy * yy;
        const float r = cull_sqrt(rr > 0.0f ? rr : 0.0f);
        *axisD = r;
        const float xx = __builtin_fmaxf(r - P.res[0], 0.0f);
        const float k = xx > 0.0f ? xx * cull_rcp(r) : 0.0f;  // e = its radial part + its axial part
        const float ya = yy > 0.0f ? __builtin_fmaxf(yy - P.res[1], 0.0f) : yy;
        ev[0] = __builtin_fabsf(k * (px - yy * P.dir[0]) + ya * P.dir[0]);
        ev[1] = __builtin_fabsf(k * (py - yy * P.dir[1]) + ya * P.dir[1]);
        ev[2] = __builtin_fabsf(k * (pz - yy * P.dir[2]) + ya * P.dir[2]);
        d2 = xx * xx + ya * ya;
    } else if (TYPE == PSGPU_T_CUBE) {
        ev[0] = __builtin_fmaxf(__builtin_fabsf(x - P.pos[0]) - P.res[0], 0.0f);
        ev[1] = __builtin_fmaxf(__builtin_fabsf(y - P.pos[1]) - P.res[0], 0.0f);
        ev[2] = __builtin_fmaxf(__builtin_fabsf(z - P.pos[2]) - P.res[0], 0.0f);
        d2 = ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2];
    }
    return cull_sqrt(d2);
}

PSGPU_HDI float wyvill_of_dist(float d) {
    const float t = 1.0f - d * d;
    return t > 0.0f ? (t * t) * t : 0.0f;
}

// Field interval of one primitive (TYPE: Point, Line, Cylinder or Cube) over the box with centre
// c, half-diagonal h and half-extents hx, hy, hz (all with their slack).  A Cylinder within 0.05 of its
// own axis (where the reference's sqrt of a rounded-negative value is NaN) clears *ok.
template <int TYPE, class PR>
PSGPU_HDI void prim_interval(PR& P, float cx, float cy, float cz, float h, float hx, float hy, float hz, float* lo,
                             float* hi, bool* ok) {
    float axisD = 1e30f, ev[3];
    const float d = prim_true_dist<TYPE, PR>(P, cx, cy, cz, &axisD, ev);
    if (TYPE == PSGPU_T_CYLINDER) *ok = *ok && (axisD - h > 0.05f);
    const float reach = (hx * ev[0] + hy * ev[1] + hz * ev[2]) * cull_rcp(d);
    float loD = __builtin_fmaxf(d - h, d - reach);
    const float ux = ev[0] + hx, uy = ev[1] + hy, uz = ev[2] + hz;
    const float hiD = __builtin_fminf(d + h, cull_sqrt(ux * ux + uy * uy + uz * uz));
    if (TYPE == PSGPU_T_POINT || TYPE == PSGPU_T_CUBE) {
        const float gx = __builtin_fmaxf(ev[0] - hx, 0.0f);
        const float gy = __builtin_fmaxf(ev[1] - hy, 0.0f);
        const float gz = __builtin_fmaxf(ev[2] - hz, 0.0f);
        loD = __builtin_fmaxf(loD, cull_sqrt(gx * gx + gy * gy + gz * gz));
    }
    *hi = wyvill_of_dist(__builtin_fmaxf(loD, 0.0f)) + kBoundEps;
    *lo = wyvill_of_dist(hiD) - kBoundEps;
}

// The S1 corner box of the 2x2x2 brick of MPUs (bi, bj, bk) (brick coordinates of the lattice),
// from the expressions precheck_body evaluates: the low face is the origin lo + (float)i * side
// of the brick's lowest MPU, the high face side + origin of its highest one, where an MPU past
// the lattice's high face is clamped to the last one.  The same bits as the minimum and maximum
// of the wave's 64 corners (both expressions are monotone in the MPU index).
PSGPU_HDI void brick_box(const float lo[3], float side, const uint32_t dims[3], uint32_t bi, uint32_t bj,
                               uint32_t bk, float blo[3], float bhi[3]) {
    const uint32_t b[3] = {bi, bj, bk};
    for (int a = 0; a < 3; ++a) {
        const uint32_t m0 = 2u * b[a], last = dims[a] - 1u;
        const uint32_t i0 = m0 < last ? m0 : last, i1 = m0 + 1u < last ? m0 + 1u : last;
        blo[a] = lo[a] + (float)i0 * side;
        bhi[a] = side + (lo[a] + (float)i1 * side);
    }
}

// Exact m / d from a multiply-high by magic = floor((2^32 - 1) / d): the estimate never exceeds
// the quotient and falls short of it by at most 2 (tests/cpp/divby_check.cpp).
PSGPU_HDI uint32_t div_by(uint32_t m, uint32_t d, uint32_t magic, uint32_t* rem) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t q = __umulhi(m, magic);
#else
    uint32_t q = (uint32_t)(((uint64_t)m * magic) >> 32);
#endif
    uint32_t r = m - q * d;
    if (r >= d) { ++q; r -= d; }
    if (r >= d) { ++q; r -= d; }
    *rem = r;
    return q;
}

struct DevModel {
    uint32_t nInstr;
    uint32_t nSlots;
    uint32_t ctPrims;
    uint32_t ctOps;
    uint32_t boundable;  // 1: field bounds over a box are valid (see prim_bound, psgpu_device.h)
    uint32_t pad[3];
    Instr instr[kMaxInstr];
    DevOp ops[128];
    DevPrim prims[128];
    CullSeg cull[128];
    float zeroCol[128][4];  // colour of op i when every field below it is +0 (see host)
    uint64_t rootZero[2];   // the primitives that, all culled over a box, make the root exactly +0
                            // there (zero_subtree_set of the root; k_sieve) ...
    uint32_t rootZeroValid; // ... and whether there is such a set (else no brick is ever dead)
    uint32_t pad2;
};

#ifndef __HIPCC_RTC__
// The zero-subtree rule (host): can op `op`'s subtree be proven exactly +0 over a box from the
// culling mask alone, and if so, which primitives must be culled for it (added to m)?  A culled
// primitive is +0 at every point of the box; Blend / Union / Intersect / Dif / SmoothDif of two
// +0 children are +0, and so is a warp of a +0 left child.  False when the subtree evaluates a
// primitive no mask ever culls (a matrix, Disc, Ring, an unknown type) or an op outside those
// types (Ricci, unknown ops).  One definition for the generated walks' skip flags (Gen::zero_set,
// psgpu_jit.cpp) and the model's root-zero set (build_device_model).
inline bool prim_maybe_culled(const DevPrim& P) {
    return P.type == PSGPU_T_TRIANGLE ||
           (!P.hasMatrix && (P.type == PSGPU_T_POINT || P.type == PSGPU_T_LINE || P.type == PSGPU_T_CYLINDER ||
                             P.type == PSGPU_T_CUBE));
}
inline bool zero_subtree_set(const DevModel& M, int op, uint64_t m[2], int depth = 0) {
    const Instr* I = nullptr;
    for (uint32_t k = 0; k < M.nInstr && !I; ++k)
        if (M.instr[k].kind == kOp && M.instr[k].idx == op) I = &M.instr[k];
    if (!I || depth > 128) return false;
    const int type = I->type, kind = I->childKind;
    auto child = [&](bool isOp, int id) {
        if (isOp) return zero_subtree_set(M, id, m, depth + 1);
        if (id >= 128 || !prim_maybe_culled(M.prims[id])) return false;
        m[id >> 6] |= 1ull << (id & 63);
        return true;
    };
    if (type >= 14 && type <= 18) return child((kind & 2) != 0, I->L) && child((kind & 1) != 0, I->R);
    if (type >= 22 && type <= 25) return child((kind & 2) != 0, I->L);
    return false;
}
// The root's set: for a tree without ops (the sum of the primitives) every primitive.  A set
// with a primitive whose segment never culls (radius +inf: not eligible, or past ctPrims) is
// no use: not valid.
inline bool root_zero_set(const DevModel& M, uint64_t m[2]) {
    m[0] = m[1] = 0ull;
    bool ok = true;
    if (M.ctOps == 0) {
        for (uint32_t k = 0; k < M.nInstr; ++k) {
            const uint32_t id = M.instr[k].idx;
            if (M.instr[k].kind != kSumPrim || id >= 128 || !prim_maybe_culled(M.prims[id])) return false;
            m[id >> 6] |= 1ull << (id & 63);
        }
        ok = M.nInstr > 0;
    } else {
        ok = zero_subtree_set(M, 0, m);
    }
    for (int i = 0; ok && i < 128; ++i)
        if (((m[i >> 6] >> (i & 63)) & 1ull) && !(M.cull[i].radius < __builtin_inff())) ok = false;
    return ok;
}
#endif

// ---- S2 octant plan (DESIGN.md §4 "S2 octants").  S1's field bounds decide some of a queued
// MPU's 8 octants (4x4x4 corners each; octant c = xh | yh << 1 | zh << 2, as octant_box has it):
// `known` has bit c set when octant c is proven outside or inside.  S2 walks the others, 4 per
// pass in octant order: 16 lanes per octant, lane & 3 = z', (lane >> 2) & 3 = y', the 4 x of the
// octant per lane, so a quad of lanes is 4 consecutive z at one (x, y) -- the quads of the full
// walk's lane = y * 8 + z layout, which is what op-box pruning groups by.
PSGPU_HDI uint32_t s2_pass_count(uint32_t known) { return (8u - (uint32_t)__builtin_popcount(known & 0xffu) + 3u) >> 2; }
// The octant lane group lane >> 4 walks in pass `pass` (< s2_pass_count): undecided octant
// 4 * pass + (lane >> 4) in octant order; a group past the last one repeats the pass's first
// octant (real points; its bits are dropped: s2_group_walks).
PSGPU_HDI uint32_t s2_plan_octant(uint32_t known, uint32_t pass, uint32_t lane) {
    uint32_t u = ~known & 0xffu;
    for (uint32_t i = 0; i < 4u * pass; ++i) u &= u - 1u;
    uint32_t v = u;
    for (uint32_t i = 0; i < 3u; ++i)
        if (i < (lane >> 4)) v &= v - 1u;
    return (uint32_t)__builtin_ctz((v ? v : u) | 0x100u) & 7u;
}
PSGPU_HDI bool s2_group_walks(uint32_t known, uint32_t pass, uint32_t lane) {
    return 4u * pass + (lane >> 4) < 8u - (uint32_t)__builtin_popcount(known & 0xffu);
}
// The inside bits ins[x] (bit y * 8 + z) of the x-slices of half xh, from the octants proven inside
PSGPU_HDI uint64_t s2_inside_const(uint32_t inside8, uint32_t xh) {
    uint64_t r = 0ull;
    for (uint32_t c = xh; c < 8u; c += 2u)
        if ((inside8 >> c) & 1u) r |= 0x0f0f0f0full << (32u * ((c >> 1) & 1u) + 4u * (c >> 2));
    return r;
}
// A walked octant's 16 ballot bits of one x (bit 4 y' + z') at their place in ins[x]
PSGPU_HDI uint64_t s2_spread(uint32_t w16, uint32_t c) {
    const uint32_t r = (w16 & 0xfu) | ((w16 & 0xf0u) << 4) | ((w16 & 0xf00u) << 8) | ((w16 & 0xf000u) << 12);
    return (uint64_t)r << (32u * ((c >> 1) & 1u) + 4u * (c >> 2));
}

// Compact-mesh work records written by the MPU kernel.
// A vertex record in two arrays, so that each kernel moves only what it uses: k_mpu writes
// the key (8 B), k_vertex reads it and writes the root (8 B), k_finish reads both and
// recomputes the position from them with k_vertex's own expressions (vertex_root).
struct VertexKey {       // 8 B: MPU slot in the range, vid | edge key << 16
    uint32_t w;
    uint32_t vidKey;     // vid | key << 16, key = sx | sy<<3 | sz<<6 | axis<<9
};
struct VertexPos {       // 8 B (k_vertex): the linear root's scale on its bracketing segment
    float scale;         // (0.5 - fa) / (fb - fa)
    uint32_t iv;         // the segment [sample iv - 1, sample iv] of the edge's 4 samples (1..3)
};
// Triangle record, 8 B.  An MPU has at most 1,715 triangles and 1,344 edges (11-bit local
// ids); the record sits in queue shard w & 63 of its MPU slot w, so the slot needs only
// w >> 6 (20 bits: ranges of up to 2^26 MPUs, checked by psgpu_polygonize).
struct TriRec {
    uint32_t a;          // tlocal | (v2 >> 10) << 11 | (w >> 6) << 12
    uint32_t b;          // v0 | v1 << 11 | (v2 & 1023) << 22
};
constexpr uint32_t kMaxRangeMpus = 1u << 26;

// Device-side scalars of one polygonization.
// Work records are appended to kShards independent queues so that no single counter
// takes one returning atomic per MPU (a single word saturates at about 88 atomics/us
// on MI355X: MI355X_MICROARCH.md 'dequeue').
constexpr int kShards = 64;
constexpr uint32_t kScanItems = 2048;   // offsets scan: counts per 256-thread block per chunk
constexpr uint32_t kScanMaxBlocks = 256;
struct ShardCtr {           // one 128-B line per shard: atomics on one line serialise
    uint32_t p;             // S1 survivors appended (k_front: shards 0-7 are its 8 sub-queues)
    uint32_t v;             // vertex records appended
    uint32_t t;             // triangle records appended
    uint32_t s;             // surface MPUs (>= 1 triangle)
    uint32_t b;             // S1 survivors proven empty by field bounds (not queued)
    uint32_t s1Done;        // k_front, shards 0-7: S1 blocks of sub-queue k that published all entries
    uint32_t pad[26];
};
struct DevCounters {
    int32_t firstOverflow;   // min global MPU id with > 512 V or T (INT32_MAX: none)
    uint32_t error;          // protocol errors (bit 0: offsets-scan look-back timeout, bit 1: k_surface's
                             // wait for the scan timed out)
    uint32_t scanDone;       // k_surface: offsets-scan blocks finished (released) in this run
    uint32_t surfaceErr;     // host copy only: 2 once a k_surface wave's scan wait timed out (plain
                             // stores of one value, so no read-modify-write over PCIe); zeroed by
                             // k_precheck, never copied from the device counters by k_surface
    uint32_t epoch;          // run sequence number: the previous run's last kernel sets it to its own
                             // + 1 when it resets this set; k_front tags its queue entries with it + 1
    uint32_t liveBricks;     // k_sieve: bricks appended to the live list (Params::liveList)
    uint32_t s2Passes;       // S2 passes walked (s2_pass_count summed over the queued MPUs); counted only
                             // with PSGPU_OPT_DEBUG bit 9, otherwise 0
    uint32_t pad[25];
    ShardCtr shard[kShards];
};

constexpr int kMpusPerBlock = 4;  // k_mpu blocks are 4 waves, one per queued S1 survivor (2 per
                                  // survivor in the tree-split kernels: 2 survivors per block)
constexpr int kNumStampKernels = 4;  // k_precheck, k_mpu, k_vertex, k_finish
constexpr int kSpanLanes = 64;       // {min start, max end} pairs per kernel per run (PSGPU_OPT_SPANS)

// Kernel arguments of one polygonization (one struct, passed by value).
struct Params {
    const DevModel* __restrict__ model;
    const CubeTablesDev* __restrict__ tables;
    float cs;           // cellsize
    float side;         // cellsize * 7.0f (MPU side)
    float lo[3];        // scene bboxLo
    uint32_t dims[3];   // MPU lattice
    uint32_t divMagic[2];  // floor((2^32 - 1) / d) for d = dims[2], dims[1] * dims[2] (mpu_origin)
    uint32_t mpuBegin;
    uint32_t mpuCount;
    uint32_t cull;      // exact per-wave primitive culling enabled
    uint32_t preBlocks;     // k_precheck blocks (4 waves, one 2x2x2 brick of MPUs per wave)
    uint32_t brickI0;       // first brick row (x) touching the MPU range
    uint32_t brickDims[3];  // bricks of the range along x, y, z
    uint32_t brickStride;   // wave W takes brick (W * brickStride) mod bricks (coprime: a
                            // permutation that spreads the surface's heavy bricks over the CUs)
    // (the next three lie in one aligned 16 bytes: S1 reads them in its first instructions, and
    // a load that also covered a word needed after the walk would hold registers across it)
    uint32_t sieve;         // k_sieve ran ahead of S1: S1 wave slot W takes entry W of liveList
    uint64_t* liveList;     // k_sieve: the bricks some primitive reaches, bi | bj << 21 | bk << 42
                            // (lattice brick coordinates), ctr->liveBricks of them, in any order
    uint32_t brickMagic[2]; // floor((2^32 - 1) / d) for d = brickDims[2], brickDims[1] * brickDims[2]
    uint64_t* pq;           // kShards queues of pShardCap S1 survivors: global MPU id | its octants
                            // S1 proved outside << 32 | proved inside << 40 (QueueEntry)
    uint64_t* pqMask;       // per queue entry: the MPU box's culling mask (2 words) and its op-inside
                            // mask (2 words, op_inside_box), by k_precheck
    uint32_t pShardCap;     // 8 * ceil(precheck waves / kShards): cannot overflow
    uint32_t* fqReady;      // k_front: per queue entry, the run's tag once the entry is published
    uint32_t fqCap;         // k_front: entries per sub-queue (8 sub-queues at pq + k * fqCap)
    uint32_t mpuBlocks;     // k_mpu grid (4 waves per block, kMpusPerBlock queued survivors per block)
    uint64_t* counts;       // mpuCount: V | T << 32 per MPU of the range (0 if S1 failed)
    uint8_t* passed;        // mpuCount: 1 if the MPU passed S1 (PsMpuStats::passedPrecheck)
    uint32_t bound;         // k_precheck proves S1 survivors empty by field bounds
    uint32_t opInside;      // k_precheck makes op-inside masks (0: zero masks, every pruning test runs)
    uint64_t* mpuMasks;     // 4 * mpuCount: culling mask of each queued MPU's box + delta, then its
                            // op-inside mask (k_precheck)
    uint64_t* offs;         // mpuCount + 1: exclusive scan of counts
    uint64_t* scanStatus;   // offsets-scan look-back words of this run (zeroed by the previous run)
    uint64_t* scanStatusNext;
    uint32_t scanBlocks;    // offsets-scan blocks (the first blocks of k_vertex)
    uint32_t scanChunks;    // kScanItems chunks per scan block
    VertexKey* vk;          // kShards queues of vShardCap vertex records (keys ...
    VertexPos* vp;          // ... and roots, same indexing)
    uint32_t vShardCap;
    TriRec* tq;             // kShards queues of tShardCap records
    uint32_t tShardCap;
    float* pos;             // vCap vertices
    float* nrm;
    float* col;
    uint32_t* tris;         // tCap triangles
    uint32_t vCap, tCap;
    DevCounters* ctr;       // this run's counters (two sets alternate between runs)
    DevCounters* ctrNext;   // the next run's, reset by k_finish
    DevCounters* hostCtr;   // host-mapped copy written by k_finish
    uint32_t* totals;       // 8 words written by k_finish: MPUs, V, T, passed S1, surface MPUs,
                            // S2 MPUs, first overflow MPU, error (the parts' count exchange)
    uint64_t* stamps;       // per-wave timeline (PSGPU_OPT_STAMPS) or null: kNumStampKernels x
    uint32_t stampCap;      // stampCap records {start, end, item | hw id << 32} (s_memrealtime)
    uint64_t* spans;        // PSGPU_OPT_SPANS: this run's slot, per kernel {first wave start, last
                            // wave end} (atomic min / max of s_memrealtime), or null
    uint64_t* mpuTicks;     // PSGPU_OPT_MPU_TICKS (MPUSTATS): 4 words per MPU of the range -- its S1
                            // wave's start and end, its S2 wave's end (0: not queued), hw ids of the
                            // S1 | S2 waves << 32 (s_memrealtime) -- or null
    uint32_t slotsPerLane;  // value slots (x4 floats in colour mode)
    uint32_t debug;         // ablation switches for profiling (0 in production)
};

static_assert(__builtin_offsetof(Params, liveList) % 16 == 0 && __builtin_offsetof(Params, pq) % 16 == 0,
              "liveList and brickMagic fill one aligned 16 bytes");

}  // namespace psgpu
