/*
 * parsip_gpu.h — C-ABI of the MI355X (gfx950) BlobTree polygonizer.
 *
 * Drop-in boundary for Parsip's PS_SimdPoly hot path.  Every struct below is
 * byte-identical to the reference SoA contract so a host that fills
 * PS::SIMDPOLY::SOABlobPrims / SOABlobOps / SOABlobPrimMatrices can hand the
 * same bytes to this library:
 *
 *   reference struct                          (Parsip100/PS_SimdPoly/include/)
 *   SOABlobPrims        9,500 B  align 4      PS_Polygonizer.h:98-130
 *   SOABlobOps          5,636 B  align 4      PS_Polygonizer.h:134-154
 *   SOABlobPrimMatrices 6,148 B  align 4      PS_Polygonizer.h:161-165
 *   SOABlobBoxMatrices  8,196 B  align 4      PS_Polygonizer.h:171-175
 *   MPU                21,524 B  align 4      PS_Polygonizer.h:183-195
 *
 * Entry points (each one cites the reference interface it replaces):
 *   psgpu_count_mpus        <- CountMPUNeeded   PS_Polygonizer.h:384, .cpp:388-412
 *   psgpu_prepare_bboxes    <- PrepareBBoxes    PS_Polygonizer.h:385, .cpp:55-309
 *   psgpu_polygonize_mpus   <- Polygonize       PS_Polygonizer.h:386-391, .cpp:315-385
 *                              (blocking, fills the caller's PolyMPUs layout)
 *   psgpu_create/destroy/set_model/polygonize/finish/...
 *                           <- the same Polygonize split into a device-resident,
 *                              stream-ordered form (compact mesh stays in HBM)
 *   psgpu_translate_blobtree_type <- enum map for SimdPoly::linearizeBlobTree
 *                              (PS_HighPerformanceRender.cpp:42-364; _constSettings.h:26-38)
 *
 * Error codes keep PS_Polygonizer.h:47-50 and add explicit overflow / device codes
 * (the reference truncates at MAX_MPU_COUNT with only a printf, .cpp:355-356, and
 * never checks the 512 vertex / triangle per-MPU capacity, .cpp:785-824).
 *
 * No torch / HIP types appear in these signatures: streams are passed as void*
 * (a hipStream_t, NULL = the context's own stream).
 */
#ifndef PARSIP_GPU_H
#define PARSIP_GPU_H

#ifdef __HIPCC_RTC__  /* embedded in run-time compiled compat kernels: no system headers */
typedef __SIZE_TYPE__ size_t;
#ifndef offsetof
#define offsetof(t, m) __builtin_offsetof(t, m)
#endif
#else
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- constants (PS_Polygonizer.h:21-81) ---------------------------------- */
#define PSGPU_GRID_DIM              8      /* corners per MPU axis (GRID_DIM_8)   */
#define PSGPU_CELLS_PER_MPU         7
#define PSGPU_ISO_VALUE             0.5f
#define PSGPU_ISO_DIST              0.45420206f
#define PSGPU_NORMAL_DELTA          0.001f
#define PSGPU_MIN_CELL_SIZE         0.01f
#define PSGPU_MAX_TREE_NODES        128
#define PSGPU_PRIM_MATRIX_STRIDE    12
#define PSGPU_BOX_MATRIX_STRIDE     16
#define PSGPU_MAX_MPU_COUNT         24000  /* the reference PolyMPUs capacity     */
#define PSGPU_MAX_MPU_VERTEX_COUNT  512
#define PSGPU_MAX_MPU_TRIANGLE_COUNT 512

/* ---- return codes -------------------------------------------------------- */
#define PSGPU_RET_SUCCESS          1   /* RET_SUCCESS                              */
#define PSGPU_RET_PARAM_ERROR     -1   /* RET_PARAM_ERROR (ctPrims == 0, bad args) */
#define PSGPU_RET_NOT_ENOUGH_MEM  -2   /* RET_NOT_ENOUGH_MEM (device alloc failed)  */
#define PSGPU_RET_INVALID_BVH     -3   /* RET_INVALID_BVH (op tree not a tree)      */
#define PSGPU_RET_MPU_OVERFLOW    -4   /* more MPUs than the caller's capacity      */
#define PSGPU_RET_MPU_VT_OVERFLOW -5   /* an MPU exceeds 512 vertices / triangles   */
#define PSGPU_RET_DEVICE_ERROR    -6   /* HIP / RCCL runtime error                  */

/* ---- node types: the hot path's own ordering (PS_Polygonizer.h:84-91) ---- */
enum PsNodeType {
    PSGPU_PRIM_CYLINDER = 0, PSGPU_PRIM_DISC = 1, PSGPU_PRIM_LINE = 2, PSGPU_PRIM_POINT = 3,
    PSGPU_PRIM_RING = 4, PSGPU_PRIM_POLYGON = 5, PSGPU_PRIM_CUBE = 6, PSGPU_PRIM_TRIANGLE = 7,
    PSGPU_PRIM_CATMULLROM = 8, PSGPU_PRIM_SKELETON = 9, PSGPU_PRIM_QUADRICPOINT = 10,
    PSGPU_PRIM_FASTQPS = 11, PSGPU_PRIM_HALFPLANE = 12, PSGPU_PRIM_NULL = 13,
    PSGPU_OP_UNION = 14, PSGPU_OP_INTERSECT = 15, PSGPU_OP_DIF = 16, PSGPU_OP_SMOOTHDIF = 17,
    PSGPU_OP_BLEND = 18, PSGPU_OP_RICCIBLEND = 19, PSGPU_OP_GRADIENTBLEND = 20,
    PSGPU_OP_AFFINE = 21, PSGPU_OP_WARPTWIST = 22, PSGPU_OP_WARPTAPER = 23,
    PSGPU_OP_WARPBEND = 24, PSGPU_OP_WARPSHEAR = 25, PSGPU_OP_CACHE = 26,
    PSGPU_OP_TEXTURE = 27, PSGPU_OP_PCM = 28
};

/* ---- SoA model (byte-exact) ---------------------------------------------- */
typedef struct PsVec3f { float x, y, z; } PsVec3f;

typedef struct PsSoaBlobPrims {          /* SOABlobPrims, PS_Polygonizer.h:98-130 */
    float posX[128], posY[128], posZ[128];
    float dirX[128], dirY[128], dirZ[128];
    float resX[128], resY[128], resZ[128];
    float colorX[128], colorY[128], colorZ[128];
    float vPrimBoxLoX[128], vPrimBoxLoY[128], vPrimBoxLoZ[128];
    float vPrimBoxHiX[128], vPrimBoxHiY[128], vPrimBoxHiZ[128];
    uint8_t skeletType[128];
    uint8_t idxMatrix[128];
    PsVec3f bboxLo;
    PsVec3f bboxHi;
    uint32_t ctPrims;
} PsSoaBlobPrims;

typedef struct PsSoaBlobOps {            /* SOABlobOps, PS_Polygonizer.h:134-154 */
    uint8_t opType[128];
    uint8_t opLeftChild[128];
    uint8_t opRightChild[128];
    uint8_t opChildKind[128];            /* bit1: left is op, bit0: right is op  */
    float vBoxLoX[128], vBoxLoY[128], vBoxLoZ[128];
    float vBoxHiX[128], vBoxHiY[128], vBoxHiZ[128];
    float resX[128], resY[128], resZ[128], resW[128];
    uint32_t ctOps;
} PsSoaBlobOps;

typedef struct PsSoaPrimMatrices {       /* SOABlobPrimMatrices, :161-165 (row 0 = identity) */
    float matrix[128 * PSGPU_PRIM_MATRIX_STRIDE];
    uint32_t count;
} PsSoaPrimMatrices;

typedef struct PsSoaBoxMatrices {        /* SOABlobBoxMatrices, :171-175 */
    float matrix[128 * PSGPU_BOX_MATRIX_STRIDE];
    uint32_t count;
} PsSoaBoxMatrices;

typedef struct PsMPU {                   /* MPU, PS_Polygonizer.h:183-195 */
    float vPos[PSGPU_MAX_MPU_VERTEX_COUNT * 3];
    float vNorm[PSGPU_MAX_MPU_VERTEX_COUNT * 3];
    float vColor[PSGPU_MAX_MPU_VERTEX_COUNT * 3];
    uint16_t triangles[PSGPU_MAX_MPU_TRIANGLE_COUNT * 3];
    uint16_t ctVertices;
    uint16_t ctTriangles;
    PsVec3f bboxLo;
    uint32_t ctFieldEvals;
} PsMPU;

/* Per-MPU outcome of a run (the library's own record; the reference's MPUSTATS is
 * PsMpuProcessStats below -- a different layout). */
typedef struct PsMpuStats {
    uint32_t passedPrecheck;   /* S1 (8-corner F>0 test) passed                  */
    uint32_t ctFieldEvals;     /* 128 if S1 passed else 0 (reference counter)     */
    uint32_t ctVertices;
    uint32_t ctTriangles;
} PsMpuStats;

/* MPUSTATS (PS_Polygonizer.h:201-207) in the reference's LP64 layout: int idxThread,
 * int bIntersected, tbb_thread::id threadID (a pthread_t), tbb::tick_count tickStart,
 * tickEnd (one long long each: legacy TBB's tick_count::now() on Linux is CLOCK_REALTIME in
 * nanoseconds).  CMPUProcessor::operator() (.cpp:449-461) writes threadID, tickStart and
 * tickEnd of every MPU and leaves idxThread / bIntersected alone; so does the library
 * (psgpu_download_process_stats):
 *   tickStart  the start of the wavefront that ran the MPU's S1 (k_precheck),
 *   tickEnd    the end of the wavefront that ran its S2-S3 and made its vertex / triangle
 *              records (k_mpu), or of its S1 wave when no S2 was needed (S1 failed, or field
 *              bounds proved it surface-free); S4-S6 run batched over every MPU's records in
 *              k_vertex / k_finish (psgpu_last_kernel_times gives their spans),
 *   threadID   the hardware slot of that last wave: XCC_ID << 16 | HW_ID[15:0] (wave slot,
 *              SIMD, CU, SH, SE), the device's "thread",
 * both ticks in CLOCK_REALTIME nanoseconds, mapped from the device clock (s_memrealtime)
 * by bracketing one device clock reading with the host clock (a few microseconds). */
typedef struct PsMpuProcessStats {
    int32_t  idxThread;
    int32_t  bIntersected;
    uint64_t threadID;
    int64_t  tickStart;
    int64_t  tickEnd;
} PsMpuProcessStats;

/* Result summary of one polygonization. */
typedef struct PsMeshInfo {
    uint32_t ctMPUs;            /* MPUs in the processed range                     */
    uint32_t ctPassedPrecheck;  /* MPUs that passed S1                              */
    uint32_t ctSurfaceMPUs;     /* MPUs that produced >= 1 triangle                 */
    uint32_t ctVertices;
    uint32_t ctTriangles;
    int32_t  firstOverflowMPU;  /* global MPU id with > 512 V or T, or -1           */
    uint64_t ctLaneEvals;       /* field evaluations performed (per point)          */
    uint32_t ctFieldMPUs;       /* S1 survivors whose 8^3 field cache was evaluated
                                 * (the rest were proven empty by field bounds)     */
    uint32_t launchFlags;       /* how the run was launched: PSGPU_LAUNCH_*         */
} PsMeshInfo;
#define PSGPU_LAUNCH_TREE_SPLIT 1u  /* k_precheck / k_mpu walked the root's subtrees in two waves */
#define PSGPU_LAUNCH_SURFACE    2u  /* k_vertex + k_finish ran as one launch (k_surface)         */
#define PSGPU_LAUNCH_FRONT      4u  /* k_precheck + k_mpu ran as one launch (k_front)            */
#define PSGPU_LAUNCH_RERUN      8u  /* finish re-ran the run (grid / capacity / protocol error)  */
#define PSGPU_LAUNCH_SIEVE     16u  /* k_sieve ran ahead of S1 (no S1 wave for a dead brick)      */

/* Device-resident compact mesh of the last polygonization (pointers into the
 * context's HBM buffers; valid until the next psgpu_polygonize on the context).
 * The vertices of the w-th MPU of the processed range [mpuBegin, mpuEnd) occupy
 * [(uint32)mpuOffsets[w], (uint32)mpuOffsets[w+1]) and its triangles
 * [mpuOffsets[w] >> 32, mpuOffsets[w+1] >> 32): MPU order, i.e. exactly the reference's
 * concatenation of vMPUs[i].vPos / triangles over i (PS_Polygonizer.cpp:360-371).   */
typedef struct PsMeshDevice {
    const float*    pos;              /* ctVertices * 3, xyz interleaved           */
    const float*    nrm;              /* ctVertices * 3                            */
    const float*    col;              /* ctVertices * 3                            */
    const uint32_t* tris;             /* ctTriangles * 3, global vertex ids        */
    const uint64_t* mpuOffsets;       /* ctMPUs + 1, exclusive scan:
                                         vertexOffset | triangleOffset << 32      */
} PsMeshDevice;

typedef struct psgpu_ctx psgpu_ctx;

/* ---- host-only helpers --------------------------------------------------- */
/* CountMPUNeeded (PS_Polygonizer.cpp:388-412). */
uint32_t psgpu_count_mpus(float cellsize, const float lo[3], const float hi[3]);
/* MPU lattice dimensions along x,y,z (PS_Polygonizer.cpp:339-352). */
int psgpu_mpu_dims(float cellsize, const PsSoaBlobPrims* prims, uint32_t dims[3]);
/* PrepareBBoxes (PS_Polygonizer.cpp:55-309) with the exact iso distance
 * PSGPU_ISO_DIST instead of the reference's undefined-behaviour FastSqrt. */
int psgpu_prepare_bboxes(float cellsize, PsSoaBlobPrims* prims, PsSoaBoxMatrices* boxMatrices,
                         PsSoaBlobOps* ops);
/* _constSettings.h:26-38 code (caller / PS_BlobTree side) -> PsNodeType; -1 if none. */
int psgpu_translate_blobtree_type(int blobtreeType);
/* Marching-cubes triangle table (256 x 16, -1 padded), generated at load time. */
void psgpu_tritable(int32_t out[256 * 16]);
/* Library version string. */
const char* psgpu_version(void);

/* ---- device context ------------------------------------------------------ */
int  psgpu_create(int deviceOrdinal, psgpu_ctx** out);
/* Frees the context; waits for an in-flight compile of its model's kernels first (call
 * it before the process exits: a compile must not run while the process tears down). */
void psgpu_destroy(psgpu_ctx* ctx);
int  psgpu_device_count(void);
/* Upload a model (validates the op tree; builds the device walk program). */
int  psgpu_set_model(psgpu_ctx* ctx, const PsSoaBlobPrims* prims,
                     const PsSoaPrimMatrices* matrices, const PsSoaBlobOps* ops);
/* Enqueue a polygonization of global MPUs [mpuBegin, mpuEnd) (clamped to the
 * lattice; pass 0, UINT32_MAX for all) on `stream` (hipStream_t or NULL). Async.
 * A range (after clamping) holds fewer than 2^26 MPUs (a 4096^3-cell lattice is 2^27:
 * split it into ranges); a larger one returns PSGPU_RET_PARAM_ERROR. */
int  psgpu_polygonize(psgpu_ctx* ctx, float cellsize, uint32_t mpuBegin, uint32_t mpuEnd,
                      void* stream);
/* Wait for the last polygonize and report counts / errors.  If the output
 * buffers were too small the call re-runs the polygonization with grown buffers. */
int  psgpu_finish(psgpu_ctx* ctx, PsMeshInfo* info);
int  psgpu_mesh_device(psgpu_ctx* ctx, PsMeshDevice* out);
/* Copy the compact mesh to host arrays (any pointer may be NULL); mpuOffsets gets
 * ctMPUs + 1 entries as in PsMeshDevice. */
int  psgpu_download_mesh(psgpu_ctx* ctx, float* pos, float* nrm, float* col, uint32_t* tris,
                         uint64_t* mpuOffsets);
/* ---- watertight indexed mesh: the weld of a finished run --------------------
 * The compact mesh concatenates per-MPU meshes, so a vertex on a face shared by two MPUs
 * appears once per MPU (up to four times on an edge line), and for most cell sizes the copies
 * differ in their last bits (each MPU computes the corner from its own origin).  The weld
 * merges them by identity, not by comparing floats: input vertex gi = mpuOffsets[w] + vid
 * sits on the global lattice edge (7 i + sx, 7 j + sy, 7 k + sz, axis), (i, j, k) the MPU
 * w + mpuBegin in x-major order, and
 *   - two input vertices are one welded vertex iff their edges are equal;
 *   - welded vertices are ordered by their smallest input index and take that vertex's
 *     position, normal and colour bit for bit;
 *   - vertexMap[gi] is the welded id of gi; triangles keep their order and become
 *     vertexMap[tris] (none drops: an MPU has one vertex per edge);
 *   - seams towards MPUs outside the processed range stay open.
 * The result depends on the run alone: welding twice gives the same bytes.  A weld leaves the
 * run's own buffers (PsMeshDevice) and the context untouched; its buffers are allocated on
 * the first psgpu_weld, so a context that never welds pays nothing. */
typedef struct PsWeldInfo {
    uint32_t ctVertices;      /* welded                                              */
    uint32_t ctTriangles;     /* == the run's                                        */
    uint32_t ctInputVertices; /* the run's                                           */
    uint32_t ctSeamVertices;  /* input vertices on an MPU face                       */
} PsWeldInfo;
typedef struct PsWeldDevice {    /* valid until the next psgpu_weld / psgpu_destroy   */
    const float*    pos;         /* ctVertices * 3                                    */
    const float*    nrm;
    const float*    col;
    const uint32_t* tris;        /* ctTriangles * 3, welded vertex ids                */
    const uint32_t* vertexMap;   /* ctInputVertices entries                           */
} PsWeldDevice;
/* Weld the context's finished run on the context's stream; blocking.  PSGPU_RET_PARAM_ERROR
 * when there is no finished run: none yet, or a psgpu_set_model / psgpu_polygonize since the
 * last psgpu_finish; and when the run reported an overflow MPU (the run exceeds the reference's
 * 512 vertices / triangles per MPU and is refused; its records are complete, nothing cuts
 * them) or a lattice axis has 2^20 / 7 MPUs or more.  An empty mesh welds to an empty mesh. */
int  psgpu_weld(psgpu_ctx* ctx, PsWeldInfo* info);
/* The welded mesh in HBM / on the host (any pointer may be NULL): PSGPU_RET_PARAM_ERROR
 * before a successful psgpu_weld of the current run. */
int  psgpu_weld_device(psgpu_ctx* ctx, PsWeldDevice* out);
int  psgpu_download_weld(psgpu_ctx* ctx, float* pos, float* nrm, float* col, uint32_t* tris,
                         uint32_t* vertexMap);
/* hipEvent times (ms) of the last psgpu_weld run with PSGPU_OPT_KERNEL_TIMING set: the whole
 * weld, then its five launches; returns the count filled. */
int  psgpu_weld_times(psgpu_ctx* ctx, float* ms, int maxPhases, const char** names);

/* ---- shells of the welded mesh: topology, area and volume ---------------------------------
 * A shell is a connected component of the welded mesh: two welded vertices are connected when
 * a triangle uses both; a welded vertex in no triangle is a shell of its own with 0 triangles.
 * Shells are ordered by their smallest welded vertex id, firstVertex.
 *
 * Edges.  For every undirected edge {lo < hi} used by triangles (a triangle corner pair with
 * equal ids is no edge), f counts its uses in winding order lo->hi and b those in order hi->lo:
 *     open          f + b == 1
 *     flipped       f + b == 2 and f != b
 *     non-manifold  f + b >= 3
 *     regular       anything else
 * An edge belongs to the shell of its vertices.  A shell is closed when it has triangles and
 * no open, flipped or non-manifold edge.
 *
 * Reproducible measures.  Everything returned is a function of the welded arrays alone, area
 * and volume included: two calls give the same bytes, and meshio.shells (plain numpy) gives
 * them too.  Sums are exact integers, by this rule (IEEE double, no contraction, evaluated
 * left to right as written):
 *   1. per triangle (a, b, c), positions converted to double:
 *        u = b - a, v = c - a
 *        n  = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx)
 *        A2 = sqrt(nx nx + ny ny + nz nz)
 *        V6 = ax (by cz - bz cy) + ay (bz cx - bx cz) + az (bx cy - by cx)
 *   2. M = the largest |coordinate| over the welded vertices, k = the smallest integer with
 *      M < 2^k (0 for M = 0), L = ceil(log2(max(T, 2))), eA = 58 - 2k - L, eV = 58 - 3k - L
 *   3. a term x at scale e: y = ldexp(x, e), hi = floor(y) as int64,
 *      lo = floor((y - hi) 2^30) as int64
 *   4. hi and lo are added into two int64 accumulators per shell and term (integer atomics:
 *      any order gives the same sum)
 *   5. a shell's value is ldexp((double)sumHi, -e) + ldexp((double)sumLo, -e - 30), divided by
 *      2 for the area (A2, eA) and by 6 for the volume (V6, eV)
 *   6. the mesh totals are the integer sums of the shells' accumulators, converted once
 *   7. |u|, |v| < 2^(k+1) per coordinate, so |n| < 2^(2k+3) per coordinate,
 *      A2 < sqrt(3) 2^(2k+3) < 2^(2k+4) and |V6| < 3 2^(3k+1) < 2^(3k+3): |hi| < 2^(62-L) and
 *      0 <= lo < 2^30, so T <= 2^L terms keep every accumulator below 2^62.
 * Coordinates must be finite.  Bounding boxes are exact float minima and maxima, with -0
 * ordered below +0; those of an empty mesh are 0.  The volume is signed: > 0 for outward
 * winding, < 0 for a cavity, and meaningful when the shell is closed. */
typedef struct PsShell {
    uint32_t firstVertex, ctVertices, ctTriangles, ctEdges;
    uint32_t ctOpenEdges, ctNonManifoldEdges, ctFlippedEdges;
    int32_t  euler;                 /* V - E + T */
    double   area, volume;
    float    bboxLo[3], bboxHi[3];
} PsShell;
typedef struct PsShellsInfo {       /* the whole mesh: counts are the sums over the shells */
    uint32_t ctShells, ctClosedShells;
    uint32_t ctVertices, ctTriangles, ctEdges, ctOpenEdges, ctNonManifoldEdges, ctFlippedEdges;
    int32_t  euler;
    uint32_t reserved;
    double   area, volume;
    float    bboxLo[3], bboxHi[3];
} PsShellsInfo;
typedef struct PsShellsDevice {     /* valid until the next weld / shells call / destroy */
    const PsShell*  shells;         /* ctShells */
    const uint32_t* vertexShell;    /* welded ctVertices: shell index of each vertex */
    const uint32_t* triShell;       /* ctTriangles */
} PsShellsDevice;
/* The shells of the context's weld, on the context's stream; blocking.  PSGPU_RET_PARAM_ERROR
 * unless the current run has been welded (psgpu_weld_device's rule); a new psgpu_weld
 * invalidates the shells.  An empty weld has 0 shells.  The weld's arrays and the run are left
 * untouched.  The buffers come with the first call, grow on demand and go with psgpu_destroy:
 * a context that never asks pays nothing.  PSGPU_RET_DEVICE_ERROR if a bounded loop of a
 * kernel ran out (a triangle naming no vertex; never on a weld's own arrays). */
int  psgpu_weld_shells(psgpu_ctx* ctx, PsShellsInfo* info);
/* The shells in HBM / on the host (any pointer may be NULL): PSGPU_RET_PARAM_ERROR before a
 * successful psgpu_weld_shells of the current weld, and for a capacity below ctShells. */
int  psgpu_weld_shells_device(psgpu_ctx* ctx, PsShellsDevice* out);
int  psgpu_download_weld_shells(psgpu_ctx* ctx, PsShell* shells, uint32_t capacity, uint32_t* vertexShell,
                                uint32_t* triShell);
/* hipEvent times (ms) of the last psgpu_weld_shells with PSGPU_OPT_KERNEL_TIMING set: the
 * whole call (its two host reads included), then its ten steps; returns the count filled. */
int  psgpu_weld_shells_times(psgpu_ctx* ctx, float* ms, int maxPhases, const char** names);

/* ---- the welded mesh filtered by shell: keep, drop, compact -------------------------------
 * Shell s of the current psgpu_weld_shells result is kept iff all of these hold:
 *     mask == NULL || mask[s] != 0
 *     ctVertices  >= minVertices
 *     ctTriangles >= minTriangles
 *     area >= minArea
 *     fabs(volume) >= minAbsVolume
 *     with PSGPU_FILTER_CLOSED_ONLY:   the shell is closed (above: it has triangles and no
 *                                      open, flipped or non-manifold edge)
 *     with PSGPU_FILTER_DROP_CAVITIES: not (the shell is closed and volume < 0)
 * The comparisons are plain IEEE comparisons of the PsShell fields as stored, so the device and
 * meshio.filter_shells (plain numpy) decide identically from identical bytes.
 *
 * The filtered mesh is the stable compaction of the welded mesh:
 *   - kept vertices, in welded order, keep pos / nrm / col bit for bit;
 *   - kept triangles, in order, become vertexMap[tris] (a kept triangle's corners are kept: a
 *     triangle's shell is its vertices' shell);
 *   - vertexMap[v] is the filtered id of welded vertex v, 0xffffffff if v is dropped;
 *   - shellMap[s] is the new index of shell s, 0xffffffff if s is dropped;
 *   - shells[] holds the kept shells' PsShell records in order, firstVertex remapped through
 *     vertexMap and no other field changed.
 * Stable compaction is monotone, so shell order is preserved: the kept shells' firstVertex
 * values still increase.  Area and volume in shells[] are the values of the unfiltered call:
 * the fixed-point scales eA / eV depend on M and T of the mesh that was measured, so a fresh
 * meshio.shells of the filtered mesh equals the kept records in every integer field and
 * bounding box, and in area and volume only up to the fixed-point resolution (each of the T
 * terms is floored twice, to 2^-(e+30): below T 2^-(e+30) / 2 for the area, / 6 for the
 * volume, plus the final roundings). */
#define PSGPU_FILTER_CLOSED_ONLY   1u
#define PSGPU_FILTER_DROP_CAVITIES 2u
typedef struct PsShellFilter {      /* all zero + no mask: every shell is kept */
    uint32_t flags;                 /* PSGPU_FILTER_CLOSED_ONLY | PSGPU_FILTER_DROP_CAVITIES */
    uint32_t minVertices, minTriangles;
    uint32_t reserved;              /* must be 0 */
    double   minArea, minAbsVolume; /* finite, >= 0 */
} PsShellFilter;
typedef struct PsFilterInfo {
    uint32_t ctVertices, ctTriangles, ctShells;                /* kept */
    uint32_t ctInputVertices, ctInputTriangles, ctInputShells; /* the weld's, the shells result's */
} PsFilterInfo;
typedef struct PsFilterDevice {     /* valid until the next weld / shells / filter call / destroy */
    const float*    pos;            /* ctVertices * 3 */
    const float*    nrm;
    const float*    col;
    const uint32_t* tris;           /* ctTriangles * 3, filtered vertex ids */
    const uint32_t* vertexMap;      /* ctInputVertices */
    const uint32_t* shellMap;       /* ctInputShells */
    const PsShell*  shells;         /* ctShells */
} PsFilterDevice;
/* Filter the context's weld by the shells of its current psgpu_weld_shells result, on the
 * context's stream; blocking.  f == NULL means all zero; mask is NULL or maskCount == ctShells
 * bytes on the host (one upload).  The criteria are evaluated on the device; the host reads
 * the totals once, at the end.  PSGPU_RET_PARAM_ERROR when there is no valid shells result for
 * the current weld (psgpu_weld_shells_device's rule), when mask != NULL and maskCount !=
 * ctShells, for unknown flag bits, reserved != 0, and for a NaN, infinite or negative minArea /
 * minAbsVolume (a call refused for its arguments leaves an earlier result as it was).  A filter that keeps nothing and a filter of an empty weld succeed with an
 * empty mesh.  A new psgpu_weld or psgpu_weld_shells invalidates the filter result, as does
 * whatever invalidates those; a second filter call replaces the first.  The weld's arrays, the
 * shells and the run are left untouched.  The buffers come with the first call, grow on demand
 * and go with the weld's: a context that never filters pays nothing.  PSGPU_RET_DEVICE_ERROR if
 * a kept triangle names a dropped vertex (never on a shells result's own arrays). */
int  psgpu_weld_filter(psgpu_ctx* ctx, const PsShellFilter* f, const uint8_t* mask, uint32_t maskCount,
                       PsFilterInfo* info);
/* The filtered mesh in HBM / on the host (any pointer may be NULL): PSGPU_RET_PARAM_ERROR before
 * a successful psgpu_weld_filter of the current shells result, and for a shellCapacity below the
 * kept count. */
int  psgpu_weld_filter_device(psgpu_ctx* ctx, PsFilterDevice* out);
int  psgpu_download_weld_filter(psgpu_ctx* ctx, float* pos, float* nrm, float* col, uint32_t* tris,
                                uint32_t* vertexMap, uint32_t* shellMap, PsShell* shells, uint32_t shellCapacity);
/* hipEvent times (ms) of the last psgpu_weld_filter with PSGPU_OPT_KERNEL_TIMING set: the whole
 * call, then one entry per launch (the mask's upload with the first, the two scans as one);
 * returns the count filled. */
int  psgpu_weld_filter_times(psgpu_ctx* ctx, float* ms, int maxPhases, const char** names);

/* Per-MPU stats for every MPU in the last processed range (ctMPUs entries). */
int  psgpu_download_stats(psgpu_ctx* ctx, PsMpuStats* stats);
/* Scatter the last result into the reference PolyMPUs layout (vMPUs[0..ctMPUs)). */
int  psgpu_export_polympus(psgpu_ctx* ctx, PsMPU* mpus, uint32_t capacity, uint32_t* outCtMPUs);
/* Blocking drop-in for PS::SIMDPOLY::Polygonize: upload, run, export. */
int  psgpu_polygonize_mpus(psgpu_ctx* ctx, float cellsize, const PsSoaBlobPrims* prims,
                           const PsSoaPrimMatrices* matrices, const PsSoaBlobOps* ops,
                           PsMPU* mpus, uint32_t capacity, uint32_t* outCtMPUs,
                           PsMpuStats* statsOrNull);
/* The same with the reference's MPUSTATS* lpProcessStats (Polygonize :386-391, :379): when
 * processStats is not NULL the run records per-MPU ticks (PSGPU_OPT_MPU_TICKS for this call)
 * and processStats[0..ctMPUs) receives them as psgpu_download_process_stats gives them. */
int  psgpu_polygonize_mpus_ex(psgpu_ctx* ctx, float cellsize, const PsSoaBlobPrims* prims,
                              const PsSoaPrimMatrices* matrices, const PsSoaBlobOps* ops,
                              PsMPU* mpus, uint32_t capacity, uint32_t* outCtMPUs,
                              PsMpuStats* statsOrNull, PsMpuProcessStats* processStatsOrNull);
/* MPUSTATS of the last run (ctMPUs entries; threadID, tickStart, tickEnd written, the other
 * fields untouched, as the reference).  PSGPU_RET_PARAM_ERROR if that run did not record
 * ticks (PSGPU_OPT_MPU_TICKS was 0 when it was enqueued). */
int  psgpu_download_process_stats(psgpu_ctx* ctx, PsMpuProcessStats* out);
/* Per-wave timeline of the last polygonize (PSGPU_OPT_STAMPS > 0; the reference's
 * MPUSTATS / PrintThreadResults, PS_Polygonizer.h:201-207, .cpp:414-461, with waves for
 * threads): 4 kernels (precheck, mpu, vertex, finish) x cap records of 3 uint64:
 * start, end (100 MHz s_memrealtime ticks), item | hw id << 32 where item is the MPU a
 * k_mpu wave polygonized (0xffffffff: none) or the wave's index, hw id = HW_ID[15:0] |
 * XCC_ID << 16.  Unlaunched waves read zero; then cap x 8 words of k_mpu phase stamps
 * (PSGPU_OPT_DEBUG bit 4096; profiling only).  Pass out = NULL to query *cap. */
int  psgpu_download_stamps(psgpu_ctx* ctx, uint64_t* out, uint32_t* cap);
/* Debug export of the finished run's vertex record queue (tests, tools/batch_live.py): the 64
 * shard counts into counts[0..64) and, with recs != NULL, every record as the pair (MPU slot in
 * the range, MPU-local vertex id), shard after shard in queue order: 2 x sum(counts) words.
 * capacity is in records; PSGPU_RET_PARAM_ERROR if it is short (counts is still written). */
int  psgpu_vertex_queue(psgpu_ctx* ctx, uint32_t* counts, uint32_t* recs, uint32_t capacity);
/* Debug export of the finished run's per-MPU masks (tests): for each of the range's ctMPUs,
 * queued[w] = 1 if k_precheck queued the MPU for S2 (only those have masks) and masks[4 w ..
 * 4 w + 3] = its culling mask (2 words, bit i: primitive i) and its op-inside mask (2 words,
 * bit k: op k; PSGPU_OPT_OP_INSIDE), zeros for an MPU that was not queued or a run without
 * culling.  capacity is in MPUs; PSGPU_RET_PARAM_ERROR if it is short. */
int  psgpu_mpu_masks(psgpu_ctx* ctx, uint8_t* queued, uint64_t* masks, uint32_t capacity);
/* Debug export of the finished run's live bricks (k_sieve's list, in list order): count receives
 * their number (0 when the run took no sieve: PSGPU_LAUNCH_SIEVE), bricks (may be null) 3 words
 * per brick, its lattice brick coordinates (x, y, z: MPU coordinates / 2). */
int  psgpu_live_bricks(psgpu_ctx* ctx, uint32_t* bricks, uint32_t capacity, uint32_t* count);
/* Debug export of the finished run's count of S2 passes: S2 walks each queued MPU's octants that
 * S1's field bounds left undecided, 4 octants per pass (0, 1 or 2 passes per MPU).  Counted only
 * in a run with PSGPU_OPT_DEBUG bit 9 (512) set; 0 otherwise, and for the tree-split kernels,
 * which walk every octant.  With bit 7 (128) S2 treats every octant as undecided: 2 per MPU. */
int  psgpu_s2_passes(psgpu_ctx* ctx, uint32_t* passes);
/* Debug export of the finished run's S1 octant verdicts, read from its queue entries: for each of
 * the range's ctMPUs, oct[w] = bit c: octant c (xh | yh << 1 | zh << 2) of the MPU proven outside,
 * bit 8 + c: proven inside; 0 for an MPU that was not queued for S2.  The tree-split S1 writes
 * them too, though its S2 does not read them.  capacity is in MPUs. */
int  psgpu_mpu_octants(psgpu_ctx* ctx, uint16_t* oct, uint32_t capacity);
/* Device memory the library holds at this moment, in bytes, over every context, group, comm
 * and compatibility context of the process (pinned host memory is not counted).  Exact, unlike
 * a device's free memory, which other processes change: a leak test compares two readings. */
uint64_t psgpu_debug_device_bytes(void);
/* PrintThreadResults (PS_Polygonizer.h:393, body .cpp:414-428, counters .cpp:443-469).
 * The reference keeps one (processed, crossed) MPU count pair per TBB worker that ran an
 * MPU, accumulated over every Polygonize of the process.  Here the worker is a device
 * context: every finished run (psgpu_finish, and every call built on it: the blocking
 * psgpu_polygonize_mpus, group parts, comm ranks) adds the MPUs of its range and those with
 * ctTriangles > 0 to its context's entry; entries are enumerated in the order contexts first
 * finished a run and outlive their context.  This divides each entry by ctAttempts, stores
 * entry i into lpThreadProcessed[i] / lpThreadCrossed[i] (either may be NULL; at most
 * `capacity` entries are written: pass psgpu_thread_result_count()), prints
 * "Thread#  i, Processed MPUs p, Crossed MPUs c " lines as the reference when print != 0,
 * clears every entry, and returns the number of entries.  ctAttempts <= 0:
 * PSGPU_RET_PARAM_ERROR, nothing cleared. */
int  psgpu_print_thread_results(int ctAttempts, uint32_t* lpThreadProcessed, uint32_t* lpThreadCrossed,
                                uint32_t capacity, int print);
/* Entries psgpu_print_thread_results would report now. */
int  psgpu_thread_result_count(void);
/* Device-side timing of the last polygonize, per kernel (ms); returns count filled. */
int  psgpu_last_kernel_times(psgpu_ctx* ctx, float* ms, int maxKernels, const char** names);
/* FieldComputer::fieldValue / fieldValueAndColor on n host points (xyz interleaved):
 * mode 0 = consecutive points form the reference's 4-lane pruning groups,
 * mode 1 = every point alone (4 identical lanes), mode 2 = mode 1 + colour (n*3). */
int  psgpu_field_values(psgpu_ctx* ctx, const float* xyz, uint32_t n, int mode, float* out, float* colOut);
/* Kernel spans of the runs recorded since PSGPU_OPT_SPANS was set: *runs slots of
 * 4 kernels x {start, end} (s_memrealtime, 100 MHz); out = NULL queries *runs. */
int  psgpu_download_spans(psgpu_ctx* ctx, uint64_t* out, uint32_t* runs);

/* Set a context option (see PSGPU_OPT_*). */
int  psgpu_set_option(psgpu_ctx* ctx, int option, int64_t value);
#define PSGPU_OPT_KERNEL_TIMING 1   /* 1: record hipEvents around every kernel */
#define PSGPU_OPT_CULLING       2   /* 1: exact per-wave primitive culling (default) */
#define PSGPU_OPT_OP_INSIDE    23   /* 1 (default): k_precheck makes, beside each queued MPU's culling
                                       mask, a mask of the ops whose box holds the MPU's box along
                                       one axis; the specialised walks skip those ops' pruning tests
                                       (which cannot prune there).  0: zero masks, every test runs.
                                       Identical output; needs PSGPU_OPT_CULLING */
#define PSGPU_OPT_DEBUG         9   /* profiling ablations (bit 0: stop after S2); 0 in use;
                                       bit 20 (test hook): the next run's k_mpu grid is one
                                       block, so finish must re-run it with the full grid;
                                       bits 23 / 24 (test hooks of the blocking export): the
                                       staging past the piece flags is filled with the call's
                                       epoch before the export / the packing kernel's last
                                       block waits ~40 us before each piece;
                                       bits 25 / 26 / 27 (test hooks, the next run only):
                                       k_surface's scan blocks count themselves done ~40 us
                                       late and its waves give up waiting after a few spins /
                                       every offsets-scan look-back times out / k_front's S1
                                       blocks publish ~40 us late and its S2 waves give up
                                       after a few polls; either way finish sees the protocol
                                       error and re-runs the polygonization as separate
                                       launches (k_precheck, k_mpu, k_vertex, k_finish; a
                                       second error: -6);
                                       bit 28 (test hook): the next run starts 3 runs short of
                                       the run counter's 32-bit wrap, where the context
                                       restarts its counter sets at epoch 0 */
#define PSGPU_OPT_VERTEX_BLOCKS_PER_CU 4  /* persistent k_vertex grid, 256-thread blocks per CU; once a
                                             run of the same range has finished, the grid is fitted
                                             to its vertices (+1/8) up to this (env PSGPU_GRID_FIT=0:
                                             always the persistent grid) */
#define PSGPU_OPT_FINISH_BLOCKS_PER_CU 5  /* persistent k_finish grid (fitted the same way) */
#define PSGPU_OPT_GRAPH         7   /* 1: replay repeated launch sequences from a hipGraph (off by
                                       default: +4-5 us per polygonization on ROCm 7.2) */
#define PSGPU_OPT_CAPACITY      6   /* restart output buffers at this vertex capacity (>= 64;
                                       they grow and the run repeats when exceeded) */
#define PSGPU_OPT_BOUND        10   /* 1: k_precheck proves S1 survivors without a surface by
                                       conservative field bounds and skips their S2 (default;
                                       output unchanged; JIT kernels only) */
#define PSGPU_OPT_JIT           3   /* 0 interpreter, 1 specialised per structure (default),
                                       2 specialised with parameters baked in (a recompile per
                                       parameter change), 3 tiered: the structure kernels at once,
                                       then -- once the model has stayed unchanged for
                                       PSGPU_OPT_TIER_RUNS polygonizations -- its baked kernels,
                                       compiled on a host thread and swapped in when loaded; a
                                       set_model that changes the model returns to the structure
                                       kernels at once (no compile on an animation's frame path).
                                       Identical output in every mode */
#define PSGPU_OPT_TIER_RUNS    18   /* tier-up threshold of PSGPU_OPT_JIT 3 (default 16, >= 1) */
#define PSGPU_OPT_STAMPS       12   /* > 0: record a per-wave timeline for up to this many waves
                                       per kernel (psgpu_download_stamps); 0: off (default) */
#define PSGPU_OPT_SPANS        13   /* > 0: the next this-many runs record each kernel's span on the
                                       device clock (first wave start, last wave end; 100 MHz) */
#define PSGPU_OPT_FINISH_QUAD  14   /* k_finish layout: 0 one lane per vertex (64 per wave), 1 a quad
                                       of lanes per vertex (16 per wave), 3 a pair of lanes (32 per
                                       wave), 2 (default) the fewest vertices per wave whose waves
                                       hold the last run's vertices in one pass of the persistent
                                       grid (16 or 32; else 64: small rank shares), at most 32 for a
                                       run enqueued while no other context of the process has a run
                                       pending on the device (a blocking caller, one context queueing
                                       its frames); identical output */
#define PSGPU_OPT_VERTEX_WIDE  15   /* k_vertex layout: 0 a quad of lanes per vertex (16 per wave),
                                       1 one lane per vertex walking its 4 edge samples (64 per wave,
                                       specialised kernels only), 2 (default) 64 when the last run's
                                       vertices overfill one pass of the persistent grid at 16 per
                                       wave and other contexts of the process have runs pending on
                                       the device (contexts taking frames in turn), else 16;
                                       identical output */
#define PSGPU_OPT_TREE_SPLIT   16   /* 1: k_precheck and k_mpu walk the root's two subtrees in two
                                       waves per brick / MPU and combine them (specialised kernels,
                                       trees whose root is a binary op over two ops); 2: only for runs
                                       whose range queued at most PSGPU_OPT_SPLIT_MAX_QUEUED MPUs for
                                       S2 last time (small rank shares); 0 (default) one wave walks the
                                       whole tree.  Non-zero compiles the split kernels too (+30-45 %
                                       hiprtc time).  Identical output */
#define PSGPU_OPT_SPLIT_MAX_QUEUED 17  /* threshold of PSGPU_OPT_TREE_SPLIT 2 (default 4 per CU) */
#define PSGPU_OPT_FUSED_SURFACE 21  /* k_vertex + k_finish as one launch (quad layouts, the offsets
                                       scan released inside it): 2 (default) for runs whose last
                                       run's vertices take the quad layouts in both (small rank
                                       shares), 1 always, 0 never, 3 always with one lane per
                                       vertex for both walks (k_surface_w: full grids; measured
                                       within 1-2 % of the two launches, so not a default).  Needs
                                       the small-launch kernels, compiled with
                                       PSGPU_OPT_TREE_SPLIT != 0.  Identical output */
#define PSGPU_OPT_FRONT        22   /* k_precheck + k_mpu as one launch, S1 survivors handed to the
                                       S2 blocks of the same launch as they are published (no grid
                                       barrier): 0 two launches, 1 always (generated kernels),
                                       2 (default) when k_precheck's grid is at most 8 blocks per
                                       CU (C3 and its shares, not C5's 512^3 frame); env
                                       PSGPU_FRONT; never with PSGPU_OPT_MPU_TICKS, nor while
                                       more than 3 other contexts have runs pending on the device */
#define PSGPU_OPT_SIEVE        24   /* k_sieve ahead of S1: a 2x2x2 brick of MPUs over whose corner box
                                       every primitive the root needs is culled gets its S1 result
                                       (nothing passes) from one lane of the sieve and no S1 wave:
                                       0 (default) never, 1 whenever culling is on and the model
                                       allows it, 2 as 1 unless the run is alone on the device; env
                                       PSGPU_SIEVE; never with PSGPU_OPT_MPU_TICKS.  Identical output.
                                       Off by default: the extra launch cost C3's step more than the
                                       dead bricks' S1 waves did */
#define PSGPU_OPT_MPU_TICKS    19   /* 1: runs record per-MPU ticks for MPUSTATS
                                       (psgpu_download_process_stats); 0 (default) off */
#define PSGPU_OPT_JIT_ASYNC    11   /* 1 (default): set_model returns at once; hiprtc compiles the
                                       specialised kernels on a host thread while the interpreter
                                       serves polygonizations (bit-identical output); 0: block */
/* Host-only (no GPU): compile the model's specialised kernels with hiprtc (mode 1:
 * structure only, 2: parameters baked in; | 4: with the tree-split kernels); returns the
 * code-object size or a negative error (log receives the compiler output). */
long psgpu_jit_compile(const PsSoaBlobPrims* prims, const PsSoaPrimMatrices* matrices,
                       const PsSoaBlobOps* ops, int mode, char* log, size_t cap);
/* Host-only (no GPU): the device image of a model (psgpu::DevModel: the walk program, the
 * culling segments, the root-zero set) into out when cap holds it; returns its size in bytes
 * or a negative error.  For tests that compile psgpu_model.h as plain C++. */
long psgpu_model_image(const PsSoaBlobPrims* prims, const PsSoaPrimMatrices* matrices,
                       const PsSoaBlobOps* ops, void* out, size_t cap);
/* 1 if the current model runs on run-time specialised kernels, 0 on the interpreter. */
int  psgpu_jit_active(psgpu_ctx* ctx);
/* 1 while the current model's specialised kernels are still compiling. */
int  psgpu_jit_pending(psgpu_ctx* ctx);
/* Block until the current model's compile has finished and adopt its kernels (with
 * PSGPU_OPT_JIT 3 also a baked compile already started); returns psgpu_jit_active
 * afterwards (0: the compile failed and the interpreter stays). */
int  psgpu_jit_wait(psgpu_ctx* ctx);
/* The kernels the next run uses: 0 interpreter, 1 structure-specialised, 2 baked. */
int  psgpu_jit_tier(psgpu_ctx* ctx);
/* Generated specialised HIP source of the current model; returns its length. */
int  psgpu_jit_source(psgpu_ctx* ctx, char* buf, size_t cap);

/* Per-MPU work of the last run in lane-evaluations (8 S1 + 64 field bounds of a survivor
 * or 512 S2 cache of a queued survivor + 8 per vertex), ctMPUs entries. */
int  psgpu_mpu_costs(psgpu_ctx* ctx, uint32_t* costs);
/* Contiguous ranges of near-equal cost over n MPUs starting at global id `begin`:
 * bounds[0..parts] (bounds[0] = begin, bounds[parts] = begin + n).  Host only. */
int  psgpu_split_costs(const uint32_t* costs, uint32_t n, uint32_t parts, uint32_t begin,
                       uint32_t* bounds);

/* ---- one grid over several devices (one process) --------------------------
 * The reference's Polygonize fans the MPU list over every core in one blocking call
 * (tbb::parallel_for, PS_Polygonizer.cpp:379-382); a group fans one MPU lattice over
 * several GPUs: contiguous MPU ranges of near-equal cost, one context per device, every
 * device launched at once.  Parts concatenated in order are exactly the single-device
 * mesh (MPUs are independent: no halo).  Several parts may share a device. */
typedef struct psgpu_group psgpu_group;
typedef struct PsGroupPart {
    int32_t  device;          /* HIP ordinal (-1: another rank's device, psgpu_comm)  */
    uint32_t mpuBegin;        /* global MPU range [mpuBegin, mpuEnd)                  */
    uint32_t mpuEnd;
    uint32_t vertexBase;      /* first vertex / triangle of the part in the whole mesh */
    uint32_t triangleBase;
    uint32_t reserved;
    PsMeshInfo info;          /* the part's own counts                                 */
} PsGroupPart;

#define PSGPU_GROUP_OPT_BALANCE       100 /* range split policy (value below)           */
#define PSGPU_GROUP_BALANCE_EVEN        0 /* equal MPU counts                            */
#define PSGPU_GROUP_BALANCE_PLAN        1 /* cost split from a planning run of the whole
                                             lattice, redone when the lattice changes
                                             (default)                                  */
#define PSGPU_GROUP_BALANCE_EVERY_RUN   2 /* plan, then re-split after every finish from
                                             the costs of that run (animations)          */
#define PSGPU_GROUP_BALANCE_FIXED       3 /* the split of psgpu_group_set_split          */
#define PSGPU_GROUP_OPT_MIN_PART_MPUS 101 /* 0 (default): every part gets a range; n > 0:
                                             only the first max(1, lattice MPUs / n) parts
                                             do, the others stay empty -- a small lattice
                                             runs as one chain (EVEN / PLAN / EVERY_RUN) */

/* devices: nParts HIP ordinals (NULL: 0 .. nParts-1). */
int  psgpu_group_create(const int* devices, int nParts, psgpu_group** out);
void psgpu_group_destroy(psgpu_group* g);
int  psgpu_group_size(psgpu_group* g);
/* The context of one part (its device-resident part of the mesh, options, timing). */
psgpu_ctx* psgpu_group_context(psgpu_group* g, int part);
/* PSGPU_GROUP_OPT_BALANCE, or any PSGPU_OPT_* (applied to every part). */
int  psgpu_group_set_option(psgpu_group* g, int option, int64_t value);
int  psgpu_group_set_model(psgpu_group* g, const PsSoaBlobPrims* prims,
                           const PsSoaPrimMatrices* matrices, const PsSoaBlobOps* ops);
int  psgpu_group_jit_wait(psgpu_group* g);
/* Explicit split: bounds[0..nParts] global MPU ids, non-decreasing (policy FIXED). */
int  psgpu_group_set_split(psgpu_group* g, const uint32_t* bounds);
int  psgpu_group_get_split(psgpu_group* g, uint32_t* bounds);
/* Enqueue the whole lattice over the parts (asynchronous on every device). */
int  psgpu_group_polygonize(psgpu_group* g, float cellsize);
/* Wait for every part; totals over the parts and, if parts != NULL, nParts entries. */
int  psgpu_group_finish(psgpu_group* g, PsMeshInfo* total, PsGroupPart* parts);
/* The whole mesh to host arrays (global vertex ids and MPU offsets, as one device). */
int  psgpu_group_download_mesh(psgpu_group* g, float* pos, float* nrm, float* col, uint32_t* tris,
                               uint64_t* mpuOffsets);
/* The whole mesh in HBM of part dstPart's device (peer copies over xGMI + rebase). */
int  psgpu_group_gather(psgpu_group* g, int dstPart, PsMeshDevice* out);
/* The group's run welded into one watertight indexed mesh in HBM of part dstPart's device:
 * psgpu_weld's contract (above) over the group's global index space, where input vertex
 * gi = vertexBase[p] + mpuOffsets_p[w] + vid of part p sits on the edge of MPU w + mpuBegin_p.
 * The seams between parts close: the result equals, byte for byte, psgpu_weld of one
 * context's run over the whole range, for any number of parts and any split.  Blocking; a
 * pending run is collected first (psgpu_group_finish) and the mesh is gathered on dstPart's
 * device (the pointers of an earlier psgpu_group_gather are overwritten).
 * PSGPU_RET_PARAM_ERROR when there is no group run, dstPart is out of range, a part reported
 * an overflow MPU, a lattice axis has 2^20 / 7 MPUs or more, or a part's own run has been
 * superseded since the group's finish (a call through psgpu_group_context's pointer).  An
 * empty mesh welds to an empty mesh.  The buffers are allocated by the group's first weld,
 * grown on demand and freed by psgpu_group_destroy or a change of dstPart: a group that never
 * welds pays nothing.  Ranks in separate processes (psgpu_comm_*) and the compat mode
 * (parsip_gpu_gui.h) have no weld across their parts. */
int  psgpu_group_weld(psgpu_group* g, int dstPart, PsWeldInfo* info);
/* The welded mesh in HBM / on the host (any pointer may be NULL): PSGPU_RET_PARAM_ERROR unless
 * the group's current run has been welded; psgpu_group_set_model, psgpu_group_polygonize,
 * psgpu_group_set_split and psgpu_group_set_option(PSGPU_OPT_CAPACITY) invalidate a weld. */
int  psgpu_group_weld_device(psgpu_group* g, PsWeldDevice* out);
int  psgpu_group_download_weld(psgpu_group* g, float* pos, float* nrm, float* col, uint32_t* tris,
                               uint32_t* vertexMap);
/* hipEvent times (ms) of the last psgpu_group_weld with PSGPU_OPT_KERNEL_TIMING set on the
 * group, on the gathering device's stream: the whole weld, the gather, the parts' edge ids
 * and their copies (as far as they outlast the gather), the mark, then resolve, scan, emit
 * and map; returns the count filled. */
int  psgpu_group_weld_times(psgpu_group* g, float* ms, int maxPhases, const char** names);
/* The shells of the group's weld (psgpu_weld_shells' contract, above), on the welding part's
 * device: PSGPU_RET_PARAM_ERROR unless the group's current run has been welded; a new
 * psgpu_group_weld invalidates them; the buffers go with psgpu_group_destroy. */
int  psgpu_group_weld_shells(psgpu_group* g, PsShellsInfo* info);
int  psgpu_group_weld_shells_device(psgpu_group* g, PsShellsDevice* out);
int  psgpu_group_download_weld_shells(psgpu_group* g, PsShell* shells, uint32_t capacity, uint32_t* vertexShell,
                                      uint32_t* triShell);
int  psgpu_group_weld_shells_times(psgpu_group* g, float* ms, int maxPhases, const char** names);
/* The group's weld filtered by its shells (psgpu_weld_filter's contract, above), on the welding
 * part's device: PSGPU_RET_PARAM_ERROR unless the group's current weld has a shells result; a
 * new psgpu_group_weld or psgpu_group_weld_shells invalidates the filter result; the buffers go
 * with psgpu_group_destroy. */
int  psgpu_group_weld_filter(psgpu_group* g, const PsShellFilter* f, const uint8_t* mask, uint32_t maskCount,
                             PsFilterInfo* info);
int  psgpu_group_weld_filter_device(psgpu_group* g, PsFilterDevice* out);
int  psgpu_group_download_weld_filter(psgpu_group* g, float* pos, float* nrm, float* col, uint32_t* tris,
                                      uint32_t* vertexMap, uint32_t* shellMap, PsShell* shells,
                                      uint32_t shellCapacity);
int  psgpu_group_weld_filter_times(psgpu_group* g, float* ms, int maxPhases, const char** names);
int  psgpu_group_export_polympus(psgpu_group* g, PsMPU* mpus, uint32_t capacity, uint32_t* outCtMPUs);
/* Blocking drop-in for PS::SIMDPOLY::Polygonize over every device of the group. */
int  psgpu_group_polygonize_mpus(psgpu_group* g, float cellsize, const PsSoaBlobPrims* prims,
                                 const PsSoaPrimMatrices* matrices, const PsSoaBlobOps* ops,
                                 PsMPU* mpus, uint32_t capacity, uint32_t* outCtMPUs);

/* ---- one process per GPU: the count exchange over RCCL (xGMI) --------------
 * Every rank polygonizes its range of one split (psgpu_split_costs of the same costs on
 * every rank) on its own context; psgpu_comm_exchange all-gathers each rank's totals
 * (8 words, written by the run's last kernel) on the context's stream. */
typedef struct psgpu_comm psgpu_comm;
#define PSGPU_COMM_ID_BYTES 128
/* Rank 0 makes the id; the caller broadcasts its bytes to the other ranks. */
int  psgpu_comm_unique_id(uint8_t id[PSGPU_COMM_ID_BYTES]);
int  psgpu_comm_create(psgpu_ctx* ctx, const uint8_t id[PSGPU_COMM_ID_BYTES], int nranks, int rank,
                       psgpu_comm** out);
void psgpu_comm_destroy(psgpu_comm* comm);
/* Enqueue the all-gather of the context's last polygonization (after psgpu_polygonize). */
int  psgpu_comm_exchange(psgpu_comm* comm, psgpu_ctx* ctx);
/* The same for a rank whose range runs as a group of parts on its one device (several
 * streams): their totals are summed on part 0's stream before the all-gather. */
int  psgpu_comm_exchange_group(psgpu_comm* comm, psgpu_group* g);
/* Wait; totals over all ranks and, if parts != NULL, nranks entries (rank order).  A
 * collective: every rank calls it.  If any rank's finish re-ran its polygonization (grown
 * buffers), the ranks agree on that (all-reduce MAX of a flag) and all exchange again. */
int  psgpu_comm_result(psgpu_comm* comm, PsMeshInfo* total, PsGroupPart* parts);
/* 1 if the last psgpu_comm_result needed that second exchange (tests, diagnostics). */
int  psgpu_comm_reexchanged(psgpu_comm* comm);

#ifdef __cplusplus
} /* extern "C" */
#endif

#ifdef __cplusplus
static_assert(sizeof(PsSoaBlobPrims) == 9500, "SOABlobPrims size");
static_assert(offsetof(PsSoaBlobPrims, skeletType) == 9216, "skeletType offset");
static_assert(offsetof(PsSoaBlobPrims, idxMatrix) == 9344, "idxMatrix offset");
static_assert(offsetof(PsSoaBlobPrims, bboxLo) == 9472, "bboxLo offset");
static_assert(offsetof(PsSoaBlobPrims, ctPrims) == 9496, "ctPrims offset");
static_assert(sizeof(PsSoaBlobOps) == 5636, "SOABlobOps size");
static_assert(offsetof(PsSoaBlobOps, vBoxLoX) == 512, "vBoxLoX offset");
static_assert(offsetof(PsSoaBlobOps, resX) == 3584, "resX offset");
static_assert(offsetof(PsSoaBlobOps, ctOps) == 5632, "ctOps offset");
static_assert(sizeof(PsSoaPrimMatrices) == 6148, "SOABlobPrimMatrices size");
static_assert(sizeof(PsSoaBoxMatrices) == 8196, "SOABlobBoxMatrices size");
static_assert(sizeof(PsMPU) == 21524, "MPU size");
static_assert(offsetof(PsMPU, vNorm) == 6144, "vNorm offset");
static_assert(offsetof(PsMPU, vColor) == 12288, "vColor offset");
static_assert(offsetof(PsMPU, triangles) == 18432, "triangles offset");
static_assert(offsetof(PsMPU, ctVertices) == 21504, "ctVertices offset");
static_assert(offsetof(PsMPU, bboxLo) == 21508, "MPU bboxLo offset");
static_assert(offsetof(PsMPU, ctFieldEvals) == 21520, "ctFieldEvals offset");
static_assert(sizeof(PsMpuProcessStats) == 32, "MPUSTATS size (LP64)");
static_assert(sizeof(PsShell) == 72, "PsShell size");
static_assert(sizeof(PsShellsInfo) == 80, "PsShellsInfo size");
static_assert(sizeof(PsShellFilter) == 32, "PsShellFilter size");
static_assert(sizeof(PsFilterInfo) == 24, "PsFilterInfo size");
static_assert(offsetof(PsMpuProcessStats, threadID) == 8, "MPUSTATS threadID offset");
static_assert(offsetof(PsMpuProcessStats, tickStart) == 16, "MPUSTATS tickStart offset");
static_assert(offsetof(PsMpuProcessStats, tickEnd) == 24, "MPUSTATS tickEnd offset");
#else
_Static_assert(sizeof(PsSoaBlobPrims) == 9500, "SOABlobPrims size");
_Static_assert(sizeof(PsSoaBlobOps) == 5636, "SOABlobOps size");
_Static_assert(sizeof(PsSoaPrimMatrices) == 6148, "SOABlobPrimMatrices size");
_Static_assert(sizeof(PsSoaBoxMatrices) == 8196, "SOABlobBoxMatrices size");
_Static_assert(sizeof(PsMPU) == 21524, "MPU size");
_Static_assert(sizeof(PsShell) == 72, "PsShell size");
_Static_assert(sizeof(PsShellsInfo) == 80, "PsShellsInfo size");
_Static_assert(sizeof(PsShellFilter) == 32, "PsShellFilter size");
_Static_assert(sizeof(PsFilterInfo) == 24, "PsFilterInfo size");
#endif

#endif /* PARSIP_GPU_H */
