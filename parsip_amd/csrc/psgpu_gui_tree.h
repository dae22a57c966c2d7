// psgpu_gui_tree.h -- the compat mode's host-only half (no HIP, no hiprtc): which caller-supplied
// trees the device walk may dereference, and the per-config marching-cubes candidate tables.
// tests/cpp/gui_tree_check.cpp runs it from this header alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

#include "../../include/parsip_gpu_gui.h"

namespace psgui {

// The per-config candidate tables (psgpu_gui_device.h's Tables) from the MC table the library
// generates (tri = psgpu_tritable's 256 x 16, digest-equal to CCubeTable.h's g_triTableCache,
// which is the same table as _CellConfigTable.h's).
template <typename Tables>
void build_tables(Tables& t, const int32_t* tri) {
    memset(&t, 0, sizeof(t));
    for (int c = 0; c < 256; ++c) {
        int n = 0;
        for (int q = 0; q < 16; ++q) {
            const int e = tri[c * 16 + q];
            if (e < 0) break;
            bool first = true;
            for (int r = 0; r < q; ++r) first = first && tri[c * 16 + r] != e;
            t.cand[c][q] = (uint8_t)(e | (first ? 16 : 0) | 32);
            n++;
        }
        t.ntri[c] = (uint8_t)(n / 3);
    }
}

// What set_tree learns about a tree beyond its validity: whether it needs the extended walk
// (PCM or Instance nodes) and, for it, each operator's parent.
struct TreeShape {
    bool ext = false;
    std::vector<uint16_t> parent;
};

// Kid ids in range, no cycles (every op reached once from op 0), depth and types the walk
// supports; for PCM / Instance nodes the restrictions of PSGUI_RET_UNSUPPORTED.
inline int validate(const PsGuiPrim* P, uint32_t nP, const PsGuiOp* O, uint32_t nO, const uint32_t* K, uint32_t nK,
                    uint32_t nM, TreeShape* shape = nullptr) {
    bool ext = false;
    for (uint32_t i = 0; i < nP; ++i) {
        const int t = P[i].type;
        if (!(t == PSGUI_PRIM_POINT || t == PSGUI_PRIM_LINE || t == PSGUI_PRIM_CYLINDER || t == PSGUI_PRIM_DISC ||
              t == PSGUI_PRIM_RING || t == PSGUI_PRIM_CUBE || t == PSGUI_PRIM_TRIANGLE ||
              t == PSGUI_PRIM_QUADRICPOINT || t == PSGUI_PRIM_NULL || t == PSGUI_PRIM_INSTANCE))
            return PSGUI_RET_UNSUPPORTED;
        if (P[i].idxMtx >= nM && P[i].idxMtx != 0) return PSGPU_RET_PARAM_ERROR;
        if (t == PSGUI_PRIM_INSTANCE) {  // a resolved origin (updateInstanceNodes, :410-431)
            ext = true;
            const float id = P[i].res1[0];
            const bool isOp = P[i].res1[2] != 0.0f;
            if (!(id >= 0.0f) || id != (float)(int)id || (uint32_t)id >= (isOp ? nO : nP)) return PSGPU_RET_PARAM_ERROR;
            if (!isOp && P[(uint32_t)id].type == PSGUI_PRIM_INSTANCE) return PSGUI_RET_UNSUPPORTED;  // nested
        }
    }
    if (nO == 0) {
        if (nP && P[0].type == PSGUI_PRIM_INSTANCE && P[0].res1[2] != 0.0f) return PSGPU_RET_PARAM_ERROR;
        if (shape) shape->ext = ext;
        return nP ? PSGPU_RET_SUCCESS : PSGPU_RET_PARAM_ERROR;
    }
    std::vector<int> seen(nO, 0);
    std::vector<uint16_t> parent(nO, 0xffffu);
    std::vector<std::pair<uint32_t, int>> stack{{0u, 1}};
    while (!stack.empty()) {
        const auto [op, depth] = stack.back();
        stack.pop_back();
        if (op >= nO || seen[op]) return PSGPU_RET_INVALID_BVH;
        seen[op] = 1;
        if (depth > PSGUI_MAX_DEPTH) return PSGUI_RET_UNSUPPORTED;
        const PsGuiOp& o = O[op];
        const int t = o.type;
        if (!(t == PSGUI_OP_UNION || t == PSGUI_OP_INTERSECT || t == PSGUI_OP_DIF || t == PSGUI_OP_SMOOTHDIF ||
              t == PSGUI_OP_BLEND || t == PSGUI_OP_RICCIBLEND || t == PSGUI_OP_WARPTWIST ||
              t == PSGUI_OP_WARPTAPER || t == PSGUI_OP_WARPBEND || t == PSGUI_OP_WARPSHEAR || t == PSGUI_OP_PCM))
            return PSGUI_RET_UNSUPPORTED;
        if (o.ctKids <= 0) return PSGUI_RET_UNSUPPORTED;
        if (t == PSGUI_OP_PCM) {
            if (o.ctKids != 2) return PSGUI_RET_UNSUPPORTED;
            ext = true;
        }
        if (o.idxMtx >= nM && o.idxMtx != 0) return PSGPU_RET_PARAM_ERROR;
        if ((uint64_t)o.kidStart + (uint64_t)o.ctKids > nK) return PSGPU_RET_PARAM_ERROR;
        for (int i = 0; i < o.ctKids; ++i) {
            const uint32_t k = K[o.kidStart + i];
            const uint32_t id = k & 0xffffu;
            if (k >> 16) {
                stack.push_back({id, depth + 1});
                if (id < nO) parent[id] = (uint16_t)op;
            } else if (id >= nP) {
                return PSGPU_RET_PARAM_ERROR;
            }
        }
    }
    if (ext) {
        // per subtree, expanded through Instances: height, PCM inside, Instance inside
        // (children have larger ids than their parent in a pre-order numbering, but the
        // caller's numbering need not be one: memoised recursion over the validated tree)
        std::vector<int> height(nO, -1), hasPcm(nO, 0), hasInst(nO, 0);
        std::function<void(uint32_t)> visit = [&](uint32_t op) {
            if (height[op] >= 0) return;
            const PsGuiOp& o = O[op];
            int h = 0, pcm = o.type == PSGUI_OP_PCM, inst = 0;
            for (int i = 0; i < o.ctKids; ++i) {
                const uint32_t k = K[o.kidStart + i], id = k & 0xffffu;
                if (k >> 16) {
                    visit(id);
                    h = std::max(h, height[id]);
                    pcm |= hasPcm[id];
                    inst |= hasInst[id];
                } else if (P[id].type == PSGUI_PRIM_INSTANCE) {
                    inst = 1;
                }
            }
            height[op] = 1 + h;
            hasPcm[op] = pcm;
            hasInst[op] = inst;
        };
        visit(0);
        // nested instancing: no Instance inside an origin operator's subtree
        for (uint32_t i = 0; i < nP; ++i)
            if (P[i].type == PSGUI_PRIM_INSTANCE && P[i].res1[2] != 0.0f) {
                const uint32_t x = (uint32_t)P[i].res1[0];
                if (!seen[x]) return PSGPU_RET_INVALID_BVH;
                if (hasInst[x]) return PSGUI_RET_UNSUPPORTED;
            }
        // PCM inside a PCM's kid subtree (through Instances too); the stack depth with every
        // Instance's origin subtree counted where it sits
        std::function<int(uint32_t, int, bool)> walk = [&](uint32_t op, int depth, bool underPcm) -> int {
            const PsGuiOp& o = O[op];
            if (depth > PSGUI_MAX_DEPTH) return PSGUI_RET_UNSUPPORTED;
            if (underPcm && o.type == PSGUI_OP_PCM) return PSGUI_RET_UNSUPPORTED;
            const bool below = underPcm || o.type == PSGUI_OP_PCM;
            for (int i = 0; i < o.ctKids; ++i) {
                const uint32_t k = K[o.kidStart + i], id = k & 0xffffu;
                int rc = PSGPU_RET_SUCCESS;
                if (k >> 16) {
                    rc = walk(id, depth + 1, below);
                } else if (P[id].type == PSGUI_PRIM_INSTANCE && P[id].res1[2] != 0.0f) {
                    const uint32_t x = (uint32_t)P[id].res1[0];
                    if (below && hasPcm[x]) return PSGUI_RET_UNSUPPORTED;
                    if (depth + height[x] > PSGUI_MAX_DEPTH) return PSGUI_RET_UNSUPPORTED;
                }
                if (rc != PSGPU_RET_SUCCESS) return rc;
            }
            return PSGPU_RET_SUCCESS;
        };
        const int rc = walk(0, 1, false);
        if (rc != PSGPU_RET_SUCCESS) return rc;
    }
    if (shape) {
        shape->ext = ext;
        shape->parent.swap(parent);
    }
    return PSGPU_RET_SUCCESS;
}

// What every entry point that takes a tree checks first: an array behind each count, a matrix table, validate.
inline int check_tree(const PsGuiPrim* prims, uint32_t ctPrims, const PsGuiOp* ops, uint32_t ctOps,
                      const uint32_t* kids, uint32_t ctKids, const PsGuiMatrix* mtx, uint32_t ctMtx,
                      TreeShape* shape = nullptr) {
    if ((ctPrims && !prims) || (ctOps && !ops) || (ctKids && !kids) || !mtx || !ctMtx) return PSGPU_RET_PARAM_ERROR;
    return validate(prims, ctPrims, ops, ctOps, kids, ctKids, ctMtx, shape);
}

}  // namespace psgui
