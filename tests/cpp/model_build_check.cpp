// model_build_check.cpp -- the main path's host-only model building (parsip_amd/csrc/
// psgpu_model_build.h: build_device_model, prepare_bboxes, lattice_dims, split_costs) as a
// stand-alone host program, for tests/test_host.py.  From the header alone, with g++ and no ROCm
// include path:
//
//   g++ -std=c++17 -O2 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -I parsip_amd/csrc
//       tests/cpp/model_build_check.cpp -o model_build_check
//
// Every input struct sits in a heap allocation of exactly its size, so a read past one is the
// sanitizer's to report.  With -DMODEL_BUILD_VIA_LIBRARY (and the library linked) the same table
// runs through psgpu_model_image, psgpu_prepare_bboxes, psgpu_mpu_dims and psgpu_split_costs.
// Prints one line per case -- name, return code, and for a success a hash of the bytes produced
// (the DevModel image; the prims and ops after prepare_bboxes; the dims; the bounds) -- then "ok".
// The test compares the lines of the builds with each other and with
// tests/golden/model_build_cases.txt, recorded from the library before the code moved into the
// header.
#define PSGPU_MODEL_NO_HIP
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "psgpu_model_build.h"

namespace {

int failures = 0;
#define EXPECT(cond)                                       \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("line %d: %s\n", __LINE__, #cond); \
            ++failures;                                    \
        }                                                  \
    } while (0)

constexpr int OK = PSGPU_RET_SUCCESS, PARAM = PSGPU_RET_PARAM_ERROR, BVH = PSGPU_RET_INVALID_BVH;
using psgpu::DevModel;

uint64_t fnv(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

void report(const char* name, int code, uint64_t hash) {
    if (code == OK) std::printf("%s %d %016llx\n", name, code, (unsigned long long)hash);
    else std::printf("%s %d\n", name, code);
}

// A model in allocations of exactly the structs' sizes (zeroed: padding bytes are hashed too).
struct Model {
    std::unique_ptr<PsSoaBlobPrims> P{new PsSoaBlobPrims};
    std::unique_ptr<PsSoaPrimMatrices> M{new PsSoaPrimMatrices};
    std::unique_ptr<PsSoaBoxMatrices> B{new PsSoaBoxMatrices};
    std::unique_ptr<PsSoaBlobOps> O{new PsSoaBlobOps};

    explicit Model(uint32_t nPrims) {
        memset(P.get(), 0, sizeof(PsSoaBlobPrims));
        memset(M.get(), 0, sizeof(PsSoaPrimMatrices));
        memset(B.get(), 0, sizeof(PsSoaBoxMatrices));
        memset(O.get(), 0, sizeof(PsSoaBlobOps));
        for (uint32_t i = 0; i < 128; ++i) {  // every slot: the image holds all 128
            const int types[4] = {PSGPU_PRIM_POINT, PSGPU_PRIM_LINE, PSGPU_PRIM_CYLINDER, PSGPU_PRIM_CUBE};
            P->posX[i] = 0.25f * (float)(i % 7);
            P->posY[i] = 0.5f * (float)(i % 5);
            P->posZ[i] = 0.125f * (float)(i % 11);
            P->dirX[i] = i % 3 == 0 ? 1.0f : 0.0f;
            P->dirY[i] = i % 3 == 1 ? 1.0f : 0.0f;
            P->dirZ[i] = i % 3 == 2 ? 1.0f : 0.0f;
            P->resX[i] = 0.3f;
            P->resY[i] = 0.7f;
            P->colorX[i] = (float)i / 128.0f;
            P->colorY[i] = 1.0f - (float)i / 256.0f;
            P->colorZ[i] = 0.5f;
            P->skeletType[i] = (uint8_t)types[i % 4];
        }
        P->ctPrims = nPrims;
        for (uint32_t m = 0; m < 128; ++m) {
            for (int k = 0; k < 3; ++k) M->matrix[m * PSGPU_PRIM_MATRIX_STRIDE + 5 * k] = 1.0f + 0.01f * (float)m;
            for (int k = 0; k < 4; ++k) B->matrix[m * PSGPU_BOX_MATRIX_STRIDE + 5 * k] = 1.0f;
            B->matrix[m * PSGPU_BOX_MATRIX_STRIDE + 12] = 0.5f * (float)m;
        }
        M->count = B->count = 4;
    }
    void op(uint32_t id, int type, int kind, uint32_t L, uint32_t R) {
        O->opType[id] = (uint8_t)type;
        O->opChildKind[id] = (uint8_t)kind;
        O->opLeftChild[id] = (uint8_t)L;
        O->opRightChild[id] = (uint8_t)R;
        O->resY[id] = 2.0f;
    }
    // ops 0 .. n-1, each the left child of the one before, with primitive right children
    void left_chain(uint32_t n) {
        for (uint32_t i = 0; i < n; ++i)
            op(i, i % 2 ? PSGPU_OP_BLEND : PSGPU_OP_UNION, i + 1 < n ? 2 : 0, i + 1 < n ? i + 1 : i % 128, (i + 1) % 128);
        O->ctOps = n;
    }
    // `levels` ops down the left, each with a leaf op as its right child: the value slots grow by
    // one a level (2 levels ops in all)
    void comb(uint32_t levels) {
        for (uint32_t i = 0; i < levels; ++i) {
            const bool last = i + 1 == levels;
            op(2 * i, PSGPU_OP_UNION, last ? 1 : 3, last ? 1 : 2 * (i + 1), 2 * i + 1);
            op(2 * i + 1, PSGPU_OP_BLEND, 0, i % 128, (i + 7) % 128);
        }
        O->ctOps = 2 * levels;
    }
};

int image(const char* name, const Model& m, DevModel* keep = nullptr) {
    std::unique_ptr<DevModel> D(new DevModel);
#ifdef MODEL_BUILD_VIA_LIBRARY
    memset(D.get(), 0, sizeof(DevModel));
    const long n = psgpu_model_image(m.P.get(), m.M.get(), m.O.get(), D.get(), sizeof(DevModel));
    EXPECT(n < 0 || n == (long)sizeof(DevModel));
    const int rc = n < 0 ? (int)n : OK;
#else
    const int rc = psgpu::build_device_model(*m.P, *m.M, *m.O, *D);
#endif
    report(name, rc, fnv(D.get(), sizeof(DevModel)));
    if (keep && rc == OK) *keep = *D;
    return rc;
}

int boxes(const char* name, Model& m, bool withBM = true) {
#ifdef MODEL_BUILD_VIA_LIBRARY
    const int rc = psgpu_prepare_bboxes(0.05f, m.P.get(), withBM ? m.B.get() : nullptr, m.O.get());
#else
    const int rc = psgpu::prepare_bboxes(m.P.get(), withBM ? m.B.get() : nullptr, m.O.get());
#endif
    report(name, rc, fnv(m.O.get(), sizeof(PsSoaBlobOps), fnv(m.P.get(), sizeof(PsSoaBlobPrims))));
    return rc;
}

void dims(const char* name, float cs, float lo, float hi, uint32_t want) {
    std::unique_ptr<PsSoaBlobPrims> P(new PsSoaBlobPrims);
    memset(P.get(), 0, sizeof(PsSoaBlobPrims));
    P->bboxLo = PsVec3f{lo, lo, lo};
    P->bboxHi = PsVec3f{hi, hi + cs, hi};  // y: one cell more
    uint32_t d[3] = {99, 99, 99};
#ifdef MODEL_BUILD_VIA_LIBRARY
    EXPECT(psgpu_mpu_dims(cs, P.get(), d) == OK);
#else
    psgpu::lattice_dims(cs, P->bboxLo, P->bboxHi, d);
#endif
    EXPECT(d[0] == want && d[2] == want);
    std::printf("%s %d %u %u %u\n", name, OK, d[0], d[1], d[2]);
}

int split(const char* name, std::initializer_list<uint32_t> costs, uint32_t parts, uint32_t begin,
          std::initializer_list<uint32_t> want = {}) {
    const uint32_t n = (uint32_t)costs.size();
    std::unique_ptr<uint32_t[]> c(n ? new uint32_t[n] : nullptr);
    std::copy(costs.begin(), costs.end(), c.get());
    std::unique_ptr<uint32_t[]> b(new uint32_t[parts + 1]);
#ifdef MODEL_BUILD_VIA_LIBRARY
    const int rc = psgpu_split_costs(c.get(), n, parts, begin, b.get());
#else
    const int rc = psgpu::split_costs(c.get(), n, parts, begin, b.get());
#endif
    report(name, rc, rc == OK ? fnv(b.get(), 4 * (parts + 1)) : 0);
    if (rc == OK && want.size()) {
        EXPECT(want.size() == parts + 1);
        EXPECT(std::equal(want.begin(), want.end(), b.get()));
    }
    return rc;
}

void images() {
    {  // the counts
        Model m(0);
        EXPECT(image("prims0", m) == PARAM);
        m.P->ctPrims = 129;
        EXPECT(image("prims129", m) == PARAM);
        m.P->ctPrims = 128;
        EXPECT(image("prims128", m) == OK);
        m.O->ctOps = 129;
        EXPECT(image("ops129", m) == PARAM);
    }
    {  // no ops: the sum program
        Model m(5);
        DevModel D;
        EXPECT(image("sum5", m, &D) == OK);
        EXPECT(D.nInstr == 5 && D.nSlots == 1 && D.ctOps == 0);
        for (uint32_t i = 0; i < 5; ++i) EXPECT(D.instr[i].kind == psgpu::kSumPrim && D.instr[i].idx == i);
    }
    {  // not a tree
        Model m(8);
        m.left_chain(3);
        EXPECT(image("chain3", m) == OK);
        m.op(1, PSGPU_OP_UNION, 2, 0, 1);  // a cycle back to the root
        EXPECT(image("cycle_root", m) == BVH);
        m.op(1, PSGPU_OP_UNION, 2, 3, 1);  // a child op id == ctOps
        EXPECT(image("child_op_ctops", m) == BVH);
        m.op(1, PSGPU_OP_UNION, 2, 127, 1);
        EXPECT(image("child_op_127", m) == BVH);
        m.op(0, PSGPU_OP_UNION, 3, 1, 1);  // op 1 reached twice
        m.op(1, PSGPU_OP_UNION, 0, 2, 3);
        EXPECT(image("op_twice", m) == BVH);
    }
    {   // A left chain: its ops share value slot 0 and take at most 3 instructions each, so neither
        // kMaxSlots nor kMaxInstr binds, and depth 127 is reached exactly by the 128 ops the SoA
        // holds: the op table is the binding limit, and one longer is a PARAM_ERROR.
        Model m(128);
        DevModel D;
        m.left_chain(128);
        EXPECT(image("left_chain128", m, &D) == OK);
        EXPECT(D.nInstr == 128 * 2 + 1 + 124 && D.nInstr <= (uint32_t)psgpu::kMaxInstr && D.nSlots == 2);
        m.O->ctOps = 129;
        EXPECT(image("left_chain129", m) == PARAM);
    }
    {   // A comb (every level's right child a leaf op): a slot more a level, and the slots bind --
        // level h needs h + 3 < kMaxSlots, so 61 levels are the deepest accepted.
        Model m(128);
        DevModel D;
        m.comb(61);
        EXPECT(image("comb61", m, &D) == OK);
        EXPECT(D.nSlots == 62 && D.nInstr <= (uint32_t)psgpu::kMaxInstr);
        Model m2(128);
        m2.comb(62);
        EXPECT(image("comb62", m2) == BVH);
    }
    {  // a primitive child id of 128
        for (int side = 0; side < 2; ++side) {
            Model m(8);
            m.left_chain(2);
            if (side) m.op(1, PSGPU_OP_UNION, 0, 128, 3);
            else m.op(1, PSGPU_OP_UNION, 0, 3, 128);
            EXPECT(image(side ? "prim128_left_union" : "prim128_right_union", m) == BVH);
            // a warp evaluates its left child only
            if (side) m.op(1, PSGPU_OP_WARPTWIST, 0, 128, 3);
            else m.op(1, PSGPU_OP_WARPTWIST, 0, 3, 128);
            EXPECT(image(side ? "prim128_left_warp" : "prim128_right_warp", m) == (side ? BVH : OK));
            // An op type that evaluates neither side (outside 14-19 and 22-25): accepted, with the
            // bytes it always had.  zero_col reads colorX/Y/Z[id] for it: for ids up to 255 that
            // is past the array but inside PsSoaBlobPrims (this program runs it under ASan).
            for (int type : {(int)PSGPU_OP_GRADIENTBLEND, (int)PSGPU_OP_TEXTURE, 0}) {
                for (uint32_t id : {128u, 255u}) {
                    if (side) m.op(1, type, 0, id, 3);
                    else m.op(1, type, 0, 3, id);
                    char name[64];
                    std::snprintf(name, sizeof(name), "prim%u_%s_type%d", id, side ? "left" : "right", type);
                    EXPECT(image(name, m) == OK);
                }
            }
        }
    }
    {  // idxMatrix
        Model m(8);
        m.left_chain(3);
        m.P->idxMatrix[2] = 127;
        EXPECT(image("matrix127", m) == OK);
        m.P->idxMatrix[2] = 128;
        EXPECT(image("matrix128", m) == PARAM);
        m.P->idxMatrix[2] = 0;
        m.P->idxMatrix[100] = 255;  // past ctPrims: every slot is uploaded
        EXPECT(image("matrix255_slot100", m) == PARAM);
    }
}

void bboxes() {
    {
        Model m(8);
        m.left_chain(4);
        m.P->idxMatrix[1] = 2;
        EXPECT(boxes("boxes_chain4", m) == OK);
    }
    {
        Model m(0);
        EXPECT(boxes("boxes_prims0", m) == PARAM);
        m.P->ctPrims = 129;
        EXPECT(boxes("boxes_prims129", m) == PARAM);
    }
    {  // an op id >= 128 on the stack
        Model m(8);
        m.left_chain(2);
        m.op(1, PSGPU_OP_UNION, 2, 128, 1);
        EXPECT(boxes("boxes_op128", m) == BVH);
        m.op(1, PSGPU_OP_UNION, 1, 1, 255);
        EXPECT(boxes("boxes_op255", m) == BVH);
    }
    {  // a two-op cycle: the guard
        Model m(8);
        m.left_chain(2);
        m.op(1, PSGPU_OP_UNION, 2, 0, 1);
        EXPECT(boxes("boxes_cycle", m) == BVH);
    }
    {  // no box matrices with a non-zero idxMatrix; idxMatrix >= BM->count: the box is not transformed
        Model m(8);
        m.left_chain(2);
        m.P->idxMatrix[0] = 3;
        EXPECT(boxes("boxes_bm_null", m, false) == OK);
        Model n(8);
        n.left_chain(2);
        n.P->idxMatrix[0] = 4;  // == count
        EXPECT(boxes("boxes_bm_count", n) == OK);
        EXPECT(memcmp(m.P.get(), n.P.get(), offsetof(PsSoaBlobPrims, idxMatrix)) == 0);
        Model k(8);
        k.left_chain(2);
        k.P->idxMatrix[0] = 3;
        EXPECT(boxes("boxes_bm_3", k) == OK);
        EXPECT(k.P->vPrimBoxLoX[0] == m.P->vPrimBoxLoX[0] + 1.5f);
    }
}

void lattice() {
    const float cs = 0.125f;  // exact in fp32, so are its multiples
    dims("dims_8cells", cs, -1.0f, -1.0f + 8.0f * cs, 2);
    dims("dims_8cells_ulp", cs, 0.0f, std::nextafter(8.0f * cs, 2.0f), 2);
    dims("dims_7cells", cs, 0.0f, 7.0f * cs, 1);
    dims("dims_7cells_ulp", cs, 0.0f, std::nextafter(7.0f * cs, 2.0f), 2);
    dims("dims_56cells", cs, 0.0f, 56.0f * cs, 8);  // a multiple of 8 cells and of 7
    dims("dims_56cells_ulp", cs, 0.0f, std::nextafter(56.0f * cs, 8.0f), 9);
    dims("dims_zero", cs, 1.0f, 1.0f, 0);
    dims("dims_negative", cs, 1.0f, 0.0f, 0);
}

void splits() {
    EXPECT(split("split_parts0", {1, 2, 3}, 0, 0) == PARAM);
    EXPECT(split("split_n0", {}, 3, 7, {7, 7, 7, 7}) == OK);
    EXPECT(split("split_zero_costs", {0, 0, 0, 0}, 2, 10) == OK);
    EXPECT(split("split_dominant", {1, 1, 1000, 1, 1}, 4, 0) == OK);
    EXPECT(split("split_even", {8, 8, 8, 8, 8, 8, 8, 8}, 4, 100, {100, 102, 104, 106, 108}) == OK);
    EXPECT(split("split_one_part", {5, 6}, 1, 3, {3, 5}) == OK);
#ifdef MODEL_BUILD_VIA_LIBRARY
    uint32_t b[2];
    EXPECT(psgpu_split_costs(nullptr, 2, 1, 0, b) == PARAM);
    EXPECT(psgpu_split_costs(nullptr, 0, 1, 0, nullptr) == PARAM);
#else
    uint32_t b[2];
    EXPECT(psgpu::split_costs(nullptr, 2, 1, 0, b) == PARAM);
    EXPECT(psgpu::split_costs(nullptr, 0, 1, 0, nullptr) == PARAM);
#endif
}

}  // namespace

int main() {
    images();
    bboxes();
    lattice();
    splits();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
