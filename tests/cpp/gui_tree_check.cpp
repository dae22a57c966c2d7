// gui_tree_check.cpp -- the compat mode's host-only half (parsip_amd/csrc/psgpu_gui_tree.h): which
// caller-supplied trees check_tree accepts, and build_tables, as a stand-alone host program for a
// run under the host sanitizers.  Linked with psgpu_gui_cull.cpp only:
//
//   g++ -std=c++17 -O2 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -I parsip_amd/csrc
//       tests/cpp/gui_tree_check.cpp parsip_amd/csrc/psgpu_gui_cull.cpp -o gui_tree_check
//   ./gui_tree_check TRITABLE      (256 x 16 integers as text: psgpu_tritable's output)
//
// Every array goes to check_tree in an allocation of exactly its stated size, so a read past an
// end is the sanitizer's to report.  The expected codes are those psgpu_gui_cull_boxes returned
// for the same arrays before validate moved into the header; with -DGUI_TREE_VIA_LIBRARY (and
// the library linked instead of psgpu_gui_cull.cpp) the same table runs through that entry point.
// Prints "ok".
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "psgpu_gui_jit.h"
#include "psgpu_gui_tree.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                       \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("line %d: %s\n", __LINE__, #cond); \
            ++failures;                                    \
        }                                                  \
    } while (0)

constexpr uint32_t OP = 1u << 16;  // a kid that is an operator
constexpr int OK = PSGPU_RET_SUCCESS, PARAM = PSGPU_RET_PARAM_ERROR, BVH = PSGPU_RET_INVALID_BVH,
              UNSUP = PSGUI_RET_UNSUPPORTED;

struct Tree {
    std::vector<PsGuiPrim> P;
    std::vector<PsGuiOp> O;
    std::vector<uint32_t> K;
    uint32_t nM = 1;  // the identity

    uint32_t prim(int type = PSGUI_PRIM_POINT) {
        PsGuiPrim p{};
        p.type = type;
        p.pos[3] = p.color[3] = 1.0f;
        P.push_back(p);
        return (uint32_t)P.size() - 1;
    }
    uint32_t inst(float origin, bool isOp) {
        const uint32_t i = prim(PSGUI_PRIM_INSTANCE);
        P[i].res1[0] = origin;
        P[i].res1[2] = isOp ? 1.0f : 0.0f;
        return i;
    }
    uint32_t op(int type, std::vector<uint32_t> kids) {  // kids may name operators that come later
        PsGuiOp o{};
        o.type = type;
        o.ctKids = (int32_t)kids.size();
        o.kidStart = (uint32_t)K.size();
        K.insert(K.end(), kids.begin(), kids.end());
        O.push_back(o);
        return (uint32_t)O.size() - 1;
    }
    // operators first .. first + n - 1, each the only kid of the one before; the last holds `leaf`
    void chain(uint32_t first, int n, uint32_t leaf) {
        for (int i = 0; i < n; ++i) {
            const uint32_t id = op(PSGUI_OP_UNION, {i + 1 < n ? (OP | (first + i + 1)) : leaf});
            EXPECT(id == first + (uint32_t)i);
        }
    }
};

template <typename T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {  // nullptr for an empty array
    std::unique_ptr<T[]> a(v.empty() ? nullptr : new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) a[i] = v[i];
    return a;
}

int run(const Tree& t) {
    const uint32_t nP = (uint32_t)t.P.size(), nO = (uint32_t)t.O.size(), nK = (uint32_t)t.K.size();
    const auto P = exact(t.P);
    const auto O = exact(t.O);
    const auto K = exact(t.K);
    std::vector<PsGuiMatrix> mv(t.nM);
    for (auto& m : mv)
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) m.r[i][j] = i == j ? 1.0f : 0.0f;
    const auto M = exact(mv);
#ifdef GUI_TREE_VIA_LIBRARY
    return psgpu_gui_cull_boxes(P.get(), nP, O.get(), nO, K.get(), nK, M.get(), t.nM, nullptr, nullptr);
#else
    psgui::TreeShape shape;
    const int rc = psgui::check_tree(P.get(), nP, O.get(), nO, K.get(), nK, M.get(), t.nM, &shape);
    if (rc == OK) {  // what set_tree does next with an accepted tree
        std::vector<float> pb, ob;
        psgui::cull_boxes(P.get(), nP, O.get(), nO, K.get(), M.get(), t.nM, pb, ob);
        EXPECT(pb.size() == 8u * nP && ob.size() == 8u * (nO ? nO : 1u));  // never an empty vector
        EXPECT(shape.parent.size() == nO);
        for (uint32_t i = 1; i < nO; ++i) EXPECT(shape.parent[i] < nO);
    }
    return rc;
#endif
}

// root union {prim 0, Instance}: the Instance's origin id as given
int instance_of(float origin, bool isOp) {
    Tree t;
    t.prim();
    t.inst(origin, isOp);
    t.op(PSGUI_OP_UNION, {0, 1});
    return run(t);
}

// An Instance under `d` nested operators, of an origin subtree `h` operators high that hangs
// off the root: the walk's stack holds d + h frames at its deepest.
int instance_depth(int d, int h) {
    Tree t;
    t.prim();
    t.inst((float)d, true);  // the origin: operator d
    t.op(PSGUI_OP_UNION, {OP | 1, OP | (uint32_t)d});
    t.chain(1, d - 1, 1);  // operators 1 .. d-1 (depths 2 .. d), the Instance below the last
    t.chain((uint32_t)d, h, 0);
    return run(t);
}

void trees() {
    {  // a bare primitive
        Tree t;
        t.prim();
        EXPECT(run(t) == OK);
    }
    {  // nothing at all
        Tree t;
        EXPECT(run(t) == PARAM);
    }
    {  // null arrays with counts, no matrix table
        PsGuiPrim p{};
        PsGuiMatrix m{};
        EXPECT(psgui::check_tree(nullptr, 1, nullptr, 0, nullptr, 0, &m, 1) == PARAM);
        EXPECT(psgui::check_tree(&p, 1, nullptr, 1, nullptr, 0, &m, 1) == PARAM);
        EXPECT(psgui::check_tree(&p, 1, nullptr, 0, nullptr, 1, &m, 1) == PARAM);
        EXPECT(psgui::check_tree(&p, 1, nullptr, 0, nullptr, 0, nullptr, 1) == PARAM);
        EXPECT(psgui::check_tree(&p, 1, nullptr, 0, nullptr, 0, &m, 0) == PARAM);
    }
    {  // a kid operator id == nO
        Tree t;
        t.prim();
        t.op(PSGUI_OP_UNION, {0, OP | 1});
        EXPECT(run(t) == BVH);
    }
    {  // a kid primitive id == nP
        Tree t;
        t.prim();
        t.op(PSGUI_OP_UNION, {0, 1});
        EXPECT(run(t) == PARAM);
    }
    {  // an operator reached twice
        Tree t;
        t.prim();
        t.op(PSGUI_OP_UNION, {OP | 1, OP | 1});
        t.op(PSGUI_OP_BLEND, {0});
        EXPECT(run(t) == BVH);
    }
    {  // a two-operator cycle
        Tree t;
        t.prim();
        t.op(PSGUI_OP_UNION, {OP | 1});
        t.op(PSGUI_OP_UNION, {0, OP | 0});
        EXPECT(run(t) == BVH);
    }
    {  // kidStart + ctKids one past nK
        Tree t;
        t.prim();
        t.op(PSGUI_OP_UNION, {0, 0});
        t.O[0].ctKids = 3;
        EXPECT(run(t) == PARAM);
        t.O[0].ctKids = 1;
        t.O[0].kidStart = 0xffffffffu;
        EXPECT(run(t) == PARAM);
        t.O[0].kidStart = 2;  // == nK
        EXPECT(run(t) == PARAM);
        t.O[0].kidStart = 1;  // the last kid
        EXPECT(run(t) == OK);
    }
    {  // no kids
        Tree t;
        t.prim();
        t.op(PSGUI_OP_UNION, {0});
        t.O[0].ctKids = 0;
        EXPECT(run(t) == UNSUP);
        t.O[0].ctKids = -1;
        EXPECT(run(t) == UNSUP);
    }
    {  // idxMtx == nM, of a primitive and of an operator
        Tree t;
        t.prim();
        t.op(PSGUI_OP_UNION, {0});
        t.nM = 2;
        t.P[0].idxMtx = 2;
        EXPECT(run(t) == PARAM);
        t.P[0].idxMtx = 1;
        EXPECT(run(t) == OK);
        t.O[0].idxMtx = 2;
        EXPECT(run(t) == PARAM);
        t.O[0].idxMtx = 1;
        EXPECT(run(t) == OK);
    }
    {  // unknown types
        Tree t;
        t.prim(5);
        t.op(PSGUI_OP_UNION, {0});
        EXPECT(run(t) == UNSUP);
        t.P[0].type = PSGUI_PRIM_POINT;
        t.O[0].type = 20;  // gradient blend
        EXPECT(run(t) == UNSUP);
        t.O[0].type = PSGUI_PRIM_POINT;
        EXPECT(run(t) == UNSUP);
    }
    for (int d : {1, PSGUI_MAX_DEPTH, PSGUI_MAX_DEPTH + 1}) {  // operator chains
        Tree t;
        t.prim();
        t.chain(0, d, 0);
        EXPECT(run(t) == (d <= PSGUI_MAX_DEPTH ? OK : UNSUP));
    }
    {  // PCM: two kids, three kids, under a PCM's kid
        Tree t;
        t.prim(), t.prim(), t.prim();
        t.op(PSGUI_OP_UNION, {OP | 1});
        t.op(PSGUI_OP_PCM, {0, 1});
        EXPECT(run(t) == OK);
        Tree t3 = t;
        t3.O[1].ctKids = 3;
        t3.K.push_back(2);
        EXPECT(run(t3) == UNSUP);
        t.K[1] = OP | 2;  // PCM {operator 2, prim 1}
        t.op(PSGUI_OP_BLEND, {OP | 3, 2});
        t.op(PSGUI_OP_PCM, {1, 2});
        EXPECT(run(t) == UNSUP);
        t.O[3].type = PSGUI_OP_BLEND;
        EXPECT(run(t) == OK);
    }
    // Instance origins
    EXPECT(instance_of(0.0f, false) == OK);
    EXPECT(instance_of(0.0f, true) == UNSUP);  // of the root: inside its own origin
    EXPECT(instance_of(-1.0f, false) == PARAM);
    EXPECT(instance_of(-1.0f, true) == PARAM);
    EXPECT(instance_of(0.5f, false) == PARAM);
    EXPECT(instance_of(NAN, false) == PARAM);
    EXPECT(instance_of(NAN, true) == PARAM);
    EXPECT(instance_of(2.0f, false) == PARAM);  // == nP
    EXPECT(instance_of(1.0f, true) == PARAM);   // == nO
    EXPECT(instance_of(1.0f, false) == UNSUP);  // itself: an Instance of an Instance
    {  // an Instance of an Instance
        Tree t;
        t.prim();
        t.inst(2.0f, false);
        t.inst(0.0f, false);
        t.op(PSGUI_OP_UNION, {0, 1, 2});
        EXPECT(run(t) == UNSUP);
    }
    {  // an Instance inside its own origin's subtree; beside it
        Tree t;
        t.prim();
        t.inst(1.0f, true);
        t.op(PSGUI_OP_UNION, {OP | 1});
        t.op(PSGUI_OP_BLEND, {0, 1});
        EXPECT(run(t) == UNSUP);
        t.K = {OP | 1, 1, 0};  // root {operator 1, the Instance}, operator 1 {prim 0}
        t.O[0].ctKids = 2;
        t.O[1].kidStart = 2;
        t.O[1].ctKids = 1;
        EXPECT(run(t) == OK);
    }
    {  // an op-origin Instance with no operators; an origin no operator reaches
        Tree t;
        t.inst(0.0f, true);
        EXPECT(run(t) == PARAM);
        Tree u;
        u.prim();
        u.inst(1.0f, true);
        u.op(PSGUI_OP_UNION, {0, 1});
        u.op(PSGUI_OP_UNION, {0});  // operator 1: in range, in no kid list
        EXPECT(run(u) == BVH);
    }
    EXPECT(instance_depth(20, 12) == OK);
    EXPECT(instance_depth(21, 12) == UNSUP);
    EXPECT(instance_depth(2, 30) == OK);
    EXPECT(instance_depth(2, 31) == UNSUP);
    EXPECT(instance_depth(31, 1) == OK);
    EXPECT(instance_depth(32, 1) == UNSUP);
}

struct Tables {  // psgpu_gui_device.h's
    uint8_t cand[256][16];
    uint8_t ntri[256];
};

void tables(const char* path) {
    std::unique_ptr<int32_t[]> tri(new int32_t[256 * 16]);
#ifdef GUI_TREE_VIA_LIBRARY
    (void)path;
    psgpu_tritable(tri.get());
#else
    FILE* f = path ? std::fopen(path, "r") : nullptr;
    EXPECT(f != nullptr);
    if (!f) return;
    int got = 0;
    for (int v; got < 256 * 16 && std::fscanf(f, "%d", &v) == 1; ++got) tri[got] = v;
    std::fclose(f);
    EXPECT(got == 256 * 16);
    if (got != 256 * 16) return;
#endif
    std::unique_ptr<Tables> t(new Tables);
    psgui::build_tables(*t, tri.get());
    int listed = 0;
    for (int c = 0; c < 256; ++c) {
        int n = 0;
        while (n < 16 && tri[c * 16 + n] >= 0) ++n;
        listed += n;
        EXPECT(n % 3 == 0 && t->ntri[c] == n / 3);
        unsigned seen = 0;
        for (int q = 0; q < 16; ++q) {
            const unsigned e = t->cand[c][q];
            if (q >= n) {
                EXPECT(e == 0);
                continue;
            }
            const unsigned edge = (unsigned)tri[c * 16 + q];
            EXPECT(edge < 12 && (e & 15u) == edge && (e & 32u));
            EXPECT(((e & 16u) != 0) == !(seen >> edge & 1u));  // bit 4: the edge's first occurrence
            seen |= 1u << edge;
        }
    }
    EXPECT(listed > 2000);  // the table is the marching-cubes one, not an empty file's
}

}  // namespace

int main(int argc, char** argv) {
    trees();
    tables(argc > 1 ? argv[1] : nullptr);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
