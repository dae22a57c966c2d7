/* psref_driver.cpp — TEST INFRASTRUCTURE ONLY.  extern "C" entry points around the compiled
 * reference (PS::SIMDPOLY of PS_Polygonizer.{h,cpp}, built in place by `make -C oracle ref`)
 * for oracle/psref.py.  The reference's structs have the layout of include/parsip_gpu.h
 * (psref_sizes lets the wrapper check that), so callers pass their SoA blocks straight in. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "PS_Polygonizer.h"

using namespace PS::SIMDPOLY;

namespace {

/* The reference loads its SIMD operands with aligned loads. */
struct Quad {
    float x[4] __attribute__((aligned(16)));
    float y[4] __attribute__((aligned(16)));
    float z[4] __attribute__((aligned(16)));
};

FieldComputer* make_computer(const void* prims, const void* mats, const void* ops) {
    void* mem = 0;
    if (posix_memalign(&mem, 64, sizeof(FieldComputer)) != 0) return 0;
    FieldComputer* fc = new (mem) FieldComputer();
    memcpy(&fc->m_blobPrims, prims, sizeof(SOABlobPrims));
    memcpy(&fc->m_blobPrimMatrices, mats, sizeof(SOABlobPrimMatrices));
    memcpy(&fc->m_blobOps, ops, sizeof(SOABlobOps));
    return fc;
}

void load(Quad& q, const float* x, const float* y, const float* z) {
    memcpy(q.x, x, sizeof q.x);
    memcpy(q.y, y, sizeof q.y);
    memcpy(q.z, z, sizeof q.z);
}

}  // namespace

extern "C" {

/* sizeof of the four input structs, MPU, PolyMPUs' MPU capacity. */
void psref_sizes(uint64_t out[6]) {
    out[0] = sizeof(SOABlobPrims);
    out[1] = sizeof(SOABlobPrimMatrices);
    out[2] = sizeof(SOABlobOps);
    out[3] = sizeof(MPU);
    out[4] = sizeof(SOABlobBoxMatrices);
    out[5] = MAX_MPU_COUNT;
}

/* Polygonize into a zeroed PolyMPUs, fresh for each run: MPUs that leave at the corner
 * precheck keep whatever counts the caller's memory held, so it has to start zeroed. */
int psref_polygonize(float cellsize, const void* prims, const void* mats, const void* ops, void** out) {
    *out = 0;
    PolyMPUs* pm = static_cast<PolyMPUs*>(calloc(1, sizeof(PolyMPUs)));
    if (!pm) return RET_NOT_ENOUGH_MEM;
    int rc = Polygonize(cellsize, *static_cast<const SOABlobPrims*>(prims),
                        *static_cast<const SOABlobPrimMatrices*>(mats), *static_cast<const SOABlobOps*>(ops), *pm);
    if (rc != RET_SUCCESS) {
        free(pm);
        return rc;
    }
    *out = pm;
    return rc;
}

void psref_result_info(const void* res, uint32_t* ctMPUs, uint32_t* ctV, uint32_t* ctT) {
    const PolyMPUs* pm = static_cast<const PolyMPUs*>(res);
    uint32_t v = 0, t = 0;
    for (uint32_t i = 0; i < pm->ctMPUs; i++) {
        v += pm->vMPUs[i].ctVertices;
        t += pm->vMPUs[i].ctTriangles;
    }
    *ctMPUs = pm->ctMPUs;
    *ctV = v;
    *ctT = t;
}

/* stats5 per MPU: passed the corner precheck (ctFieldEvals was written), ctFieldEvals,
 * ctVertices, ctTriangles, 0; the arrays are the MPUs' used parts, concatenated in MPU order.
 * origins (3 floats per MPU, optional) receives every bboxLo. */
void psref_result_copy(const void* res, uint32_t* stats5, float* pos, float* nrm, float* col, uint16_t* tri,
                       float* origins) {
    const PolyMPUs* pm = static_cast<const PolyMPUs*>(res);
    size_t v = 0, t = 0;
    for (uint32_t i = 0; i < pm->ctMPUs; i++) {
        const MPU& m = pm->vMPUs[i];
        stats5[i * 5 + 0] = m.ctFieldEvals != 0;
        stats5[i * 5 + 1] = m.ctFieldEvals;
        stats5[i * 5 + 2] = m.ctVertices;
        stats5[i * 5 + 3] = m.ctTriangles;
        stats5[i * 5 + 4] = 0;
        if (origins) {
            origins[i * 3 + 0] = m.bboxLo.x;
            origins[i * 3 + 1] = m.bboxLo.y;
            origins[i * 3 + 2] = m.bboxLo.z;
        }
        if (pos) memcpy(pos + v * 3, m.vPos, size_t(m.ctVertices) * 3 * sizeof(float));
        if (nrm) memcpy(nrm + v * 3, m.vNorm, size_t(m.ctVertices) * 3 * sizeof(float));
        if (col) memcpy(col + v * 3, m.vColor, size_t(m.ctVertices) * 3 * sizeof(float));
        if (tri) memcpy(tri + t * 3, m.triangles, size_t(m.ctTriangles) * 3 * sizeof(uint16_t));
        v += m.ctVertices;
        t += m.ctTriangles;
    }
}

void psref_result_free(void* res) { free(res); }

int psref_prepare_bboxes(float cellsize, void* prims, void* boxmats, void* ops) {
    return PrepareBBoxes(cellsize, *static_cast<SOABlobPrims*>(prims), *static_cast<SOABlobBoxMatrices*>(boxmats),
                         *static_cast<SOABlobOps*>(ops));
}

uint32_t psref_count_mpus(float cellsize, const float lo[3], const float hi[3]) {
    return CountMPUNeeded(cellsize, svec3f(lo[0], lo[1], lo[2]), svec3f(hi[0], hi[1], hi[2]));
}

/* FieldComputer::fieldValue, one 4-lane quad at a time, over n points (n a multiple of 4). */
int psref_field_value(const void* prims, const void* mats, const void* ops, uint32_t n, const float* x,
                      const float* y, const float* z, float* out) {
    FieldComputer* fc = make_computer(prims, mats, ops);
    if (!fc) return RET_NOT_ENOUGH_MEM;
    Quad q;
    float f[4] __attribute__((aligned(16)));
    for (uint32_t i = 0; i + 4 <= n; i += 4) {
        load(q, x + i, y + i, z + i);
        Float_ X(q.x), Y(q.y), Z(q.z), F;
        fc->fieldValue(X, Y, Z, F);
        F.store(f);
        memcpy(out + i, f, sizeof f);
    }
    free(fc);
    return RET_SUCCESS;
}

int psref_field_value_and_color(const void* prims, const void* mats, const void* ops, uint32_t n, const float* x,
                                const float* y, const float* z, float* out, float* cx, float* cy, float* cz) {
    FieldComputer* fc = make_computer(prims, mats, ops);
    if (!fc) return RET_NOT_ENOUGH_MEM;
    Quad q;
    float f[4] __attribute__((aligned(16)));
    for (uint32_t i = 0; i + 4 <= n; i += 4) {
        load(q, x + i, y + i, z + i);
        Float_ X(q.x), Y(q.y), Z(q.z), F, CX, CY, CZ;
        fc->fieldValueAndColor(X, Y, Z, F, CX, CY, CZ);
        F.store(f);
        memcpy(out + i, f, sizeof f);
        CX.store(f);
        memcpy(cx + i, f, sizeof f);
        CY.store(f);
        memcpy(cy + i, f, sizeof f);
        CZ.store(f);
        memcpy(cz + i, f, sizeof f);
    }
    free(fc);
    return RET_SUCCESS;
}

}  // extern "C"
