// psgpu_group_plan.h — what a group of parts decides without a GPU (psgpu_group.cpp,
// psgpu_comm.cpp): which parts get MPU ranges and when the split is redone, what the 8 k_finish
// words of a part mean, and where each part's mesh lies in the whole mesh's index space.
//
// Host only, no HIP, not embedded for hiprtc: a plain C++ program (tests/cpp/
// group_plan_check.cpp) includes it with no ROCm include path.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/parsip_gpu.h"

namespace psgpu {

// The split of a lattice's MPUs over a group's parts, and the lattice it was planned for.
struct SplitPlan {
    uint32_t parts = 0;            // the group's
    std::vector<uint32_t> bounds;  // parts + 1 global MPU ids (empty: none yet)
    int balance = PSGPU_GROUP_BALANCE_PLAN;
    uint32_t minPartMpus = 0;      // PSGPU_GROUP_OPT_MIN_PART_MPUS
    bool planned = false;          // bounds are a cost split of the lattice below
    float planCs = 0.0f;
    PsVec3f planLo{}, planHi{};

    bool have_bounds() const { return bounds.size() == (size_t)parts + 1; }
    // Parts that get a range: all, or with PSGPU_GROUP_OPT_MIN_PART_MPUS the first
    // total / minPartMpus of them (at least one); the rest get empty ranges at the end.
    uint32_t active_parts(uint32_t total) const {
        if (!minPartMpus) return parts;
        return std::max(1u, std::min(parts, total / minPartMpus));
    }
    void even_split(uint32_t total) {
        const uint32_t a = active_parts(total);
        bounds.assign((size_t)parts + 1, total);
        for (uint32_t k = 0; k < a; ++k) bounds[k] = (uint32_t)((uint64_t)total * k / a);
    }
    // The plan is of this cell size and bounding box (their bytes: -0.0 is not +0.0).
    bool same_lattice(float cs, const PsVec3f& lo, const PsVec3f& hi) const {
        return planned && planCs == cs && !memcmp(&planLo, &lo, sizeof(PsVec3f)) && !memcmp(&planHi, &hi, sizeof(PsVec3f));
    }
};

// What psgpu_group_polygonize does about the split before it launches a lattice of `total` MPUs:
// keep the bounds, split evenly, or make a planning run; and whether a pending run has to be
// finished first (the split depends on it, or runs would queue up per part stream).
enum class SplitAction { Keep, Even, Plan };
struct SplitDecision {
    bool finishFirst;
    SplitAction action;
};
inline SplitDecision decide(const SplitPlan& s, float cs, const PsVec3f& lo, const PsVec3f& hi, uint32_t total,
                            bool pending) {
    const bool same = s.same_lattice(cs, lo, hi);
    const bool replan = s.balance == PSGPU_GROUP_BALANCE_PLAN && (!same || !s.have_bounds() || s.bounds[s.parts] != total);
    const bool finishFirst = pending && (replan || s.balance == PSGPU_GROUP_BALANCE_EVERY_RUN);
    if (s.balance == PSGPU_GROUP_BALANCE_FIXED) return {finishFirst, s.have_bounds() ? SplitAction::Keep : SplitAction::Even};
    if (s.balance == PSGPU_GROUP_BALANCE_EVEN) return {finishFirst, SplitAction::Even};
    const bool plan = replan || (s.balance == PSGPU_GROUP_BALANCE_EVERY_RUN && !same);
    return {finishFirst, plan ? SplitAction::Plan : SplitAction::Keep};
}

// PsMeshInfo::ctLaneEvals of a run: 8 corner lanes an MPU, 512 a field MPU, 8 a vertex.
inline uint64_t lane_evals(uint32_t mpus, uint32_t fieldMpus, uint32_t vertices) {
    return 8ull * mpus + 512ull * fieldMpus + 8ull * vertices;
}

// The 8 words k_finish leaves of a run (Params::totals, psgpu_model.h): MPUs, vertices,
// triangles, passed S1, surface MPUs, S2 MPUs, the first overflowing MPU (0x7fffffff: none), and
// the error word, which is the caller's to test.  launchFlags are not among them: 0.
inline PsMeshInfo decode_totals(const uint32_t w[8]) {
    PsMeshInfo I;
    memset(&I, 0, sizeof(I));
    I.ctMPUs = w[0];
    I.ctVertices = w[1];
    I.ctTriangles = w[2];
    I.ctPassedPrecheck = w[3];
    I.ctSurfaceMPUs = w[4];
    I.ctFieldMPUs = w[5];
    I.firstOverflowMPU = w[6] == 0x7fffffffu ? -1 : (int32_t)w[6];
    I.ctLaneEvals = lane_evals(w[0], w[5], w[1]);
    return I;
}

// The count exchange: each of n parts' place in the whole mesh's index space (vBase, tBase: n
// words each) and the totals over them -- the sums, any part's launchFlags, the first part's
// overflowing MPU.  PSGPU_RET_NOT_ENOUGH_MEM when the vertices or the triangles pass 2^32 - 1
// (*total then holds neither count).
inline int place_parts(const PsMeshInfo* info, size_t n, uint32_t* vBase, uint32_t* tBase, PsMeshInfo* total) {
    PsMeshInfo& T = *total;
    memset(&T, 0, sizeof(T));
    T.firstOverflowMPU = -1;
    uint64_t v = 0, t = 0;
    for (size_t p = 0; p < n; ++p) {
        const PsMeshInfo& I = info[p];
        vBase[p] = (uint32_t)v;
        tBase[p] = (uint32_t)t;
        v += I.ctVertices;
        t += I.ctTriangles;
        T.ctMPUs += I.ctMPUs;
        T.ctPassedPrecheck += I.ctPassedPrecheck;
        T.ctSurfaceMPUs += I.ctSurfaceMPUs;
        T.ctLaneEvals += I.ctLaneEvals;
        T.ctFieldMPUs += I.ctFieldMPUs;
        T.launchFlags |= I.launchFlags;
        if (I.firstOverflowMPU >= 0 && T.firstOverflowMPU < 0) T.firstOverflowMPU = I.firstOverflowMPU;
    }
    if (v > 0xffffffffull || t > 0xffffffffull) return PSGPU_RET_NOT_ENOUGH_MEM;
    T.ctVertices = (uint32_t)v;
    T.ctTriangles = (uint32_t)t;
    return PSGPU_RET_SUCCESS;
}

// A part's MPU offsets in the whole mesh's: its ctMPUs + 1 words go to word mBase on (the MPUs
// of the parts before it; its last word is the next part's first) with `add` added, its vertex
// base in the low half and its triangle base in the high one.  False: no part has an MPU, so no
// part writes word 0, which the caller then zeroes.
struct OffsetRebase {
    uint64_t mBase, add;
};
inline bool offset_rebases(const PsMeshInfo* info, const uint32_t* vBase, const uint32_t* tBase, size_t n,
                           OffsetRebase* out) {
    uint64_t mBase = 0;
    for (size_t p = 0; p < n; ++p) {
        out[p] = {mBase, (uint64_t)vBase[p] | ((uint64_t)tBase[p] << 32)};
        mBase += info[p].ctMPUs;
    }
    return mBase != 0;
}

}  // namespace psgpu
