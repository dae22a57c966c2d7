// group_plan_check.cpp -- what a group of parts decides without a GPU (parsip_amd/csrc/
// psgpu_group_plan.h: SplitPlan, decide, decode_totals, place_parts) as a stand-alone host
// program, for tests/test_host.py.  From the headers alone, with g++ and no ROCm include path:
//
//   g++ -std=c++17 -O2 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=all -I parsip_amd/csrc
//       tests/cpp/group_plan_check.cpp -o group_plan_check
//
// Every array a call takes is a heap allocation of exactly its stated size, so an access past one
// is the sanitizer's to report.  Prints one line per case, then "ok"; the test compares the lines
// with tests/golden/group_plan_cases.txt, recorded from the bodies of psgpu_group.cpp's entry
// points before this code moved into the header.
#define PSGPU_MODEL_NO_HIP
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "psgpu_plan.h"

namespace {

// The code under test, behind the few calls the cases make.
using Plan = psgpu::SplitPlan;
uint32_t active_parts(const Plan& s, uint32_t total) { return s.active_parts(total); }
void even_split(Plan& s, uint32_t total) { s.even_split(total); }
void decide(const Plan& s, float cs, const PsVec3f& lo, const PsVec3f& hi, uint32_t total, bool pending, bool* finishFirst,
            const char** action) {
    const psgpu::SplitDecision d = psgpu::decide(s, cs, lo, hi, total, pending);
    *finishFirst = d.finishFirst;
    *action = d.action == psgpu::SplitAction::Keep ? "keep" : d.action == psgpu::SplitAction::Even ? "even" : "plan";
}
int place(const PsMeshInfo* info, size_t n, uint32_t* vBase, uint32_t* tBase, PsMeshInfo* total) {
    return psgpu::place_parts(info, n, vBase, tBase, total);
}
PsMeshInfo decode(const uint32_t* w) { return psgpu::decode_totals(w); }
// psgpu_comm_result's use of the two: nranks x 8 gathered words to nranks parts and the totals
int place_words(const uint32_t* words, int nranks, PsGroupPart* parts, PsMeshInfo* total) {
    std::unique_ptr<PsMeshInfo[]> info(new PsMeshInfo[nranks]);
    std::unique_ptr<uint32_t[]> vBase(new uint32_t[nranks]), tBase(new uint32_t[nranks]);
    for (int r = 0; r < nranks; ++r) info[r] = psgpu::decode_totals(words + 8 * r);
    const int rc = psgpu::place_parts(info.get(), (size_t)nranks, vBase.get(), tBase.get(), total);
    if (rc != PSGPU_RET_SUCCESS) return rc;
    uint32_t mb = 0;
    for (int r = 0; r < nranks; ++r) {
        PsGroupPart& P = parts[r];
        memset(&P, 0, sizeof(P));
        P.device = -1;
        P.mpuBegin = mb;
        P.mpuEnd = mb += info[r].ctMPUs;
        P.vertexBase = vBase[r];
        P.triangleBase = tBase[r];
        P.info = info[r];
    }
    return rc;
}

// ---- the cases ----

int failures = 0;
#define EXPECT(cond)                                       \
    do {                                                   \
        if (!(cond)) {                                     \
            std::printf("line %d: %s\n", __LINE__, #cond); \
            ++failures;                                    \
        }                                                  \
    } while (0)

void print_info(const PsMeshInfo& I) {
    std::printf(" mpus=%u passed=%u surface=%u v=%u t=%u overflow=%d evals=%llu field=%u flags=%u", I.ctMPUs,
                I.ctPassedPrecheck, I.ctSurfaceMPUs, I.ctVertices, I.ctTriangles, I.firstOverflowMPU,
                (unsigned long long)I.ctLaneEvals, I.ctFieldMPUs, I.launchFlags);
}

void even_cases() {
    const uint32_t totals[] = {0u, 1u, 7u, 8u, 9u, 0xffffffffu}, parts[] = {1, 2, 3, 8, 64};
    for (uint32_t total : totals)
        for (uint32_t n : parts) {
            const uint32_t mins[] = {0u, 1u, 4u, total, total + 1u};  // (2^32 - 1) + 1 is 0 again
            for (uint32_t m : mins) {
                Plan s;
                s.parts = n;
                s.minPartMpus = m;
                const uint32_t a = active_parts(s, total);
                even_split(s, total);
                std::printf("even total=%u parts=%u min=%u: active=%u bounds", total, n, m, a);
                for (uint32_t b : s.bounds) std::printf(" %u", b);
                std::printf("\n");
                EXPECT(a >= 1 && a <= n);
                EXPECT(s.bounds.size() == (size_t)n + 1 && s.bounds[0] == 0 && s.bounds[n] == total);
                for (uint32_t k = 0; k < n; ++k) EXPECT(s.bounds[k] <= s.bounds[k + 1]);
                // the parts past the active ones are the empty ones at the end ...
                for (uint32_t k = a; k < n; ++k) EXPECT(s.bounds[k] == total);
                // ... and with a minimum, active <= total, so every active part holds an MPU: no
                // empty part ahead of a full one.  (Without one, total < parts floors leading
                // ranges to nothing, as it always has.)
                if (m && total)
                    for (uint32_t k = 0; k < a; ++k) EXPECT(s.bounds[k] < s.bounds[k + 1]);
            }
        }
    Plan s;  // the product total * k is 64-bit: 63 (2^32 - 1) / 64
    s.parts = 64;
    even_split(s, 0xffffffffu);
    EXPECT(s.bounds[63] == 4227858431u);
}

void decide_cases() {
    const char* modes[] = {"EVEN", "PLAN", "EVERY_RUN", "FIXED"};
    const char* states[] = {"same", "cs", "bbox", "negzero", "unplanned", "nobounds", "boundsN"};
    for (int mode = 0; mode < 4; ++mode)
        for (const char* st : states)
            for (int pending = 0; pending < 2; ++pending) {
                const std::string state = st;
                Plan s;
                s.parts = 3;
                s.balance = mode;
                s.bounds = {0, 8, 16, 24};
                s.planned = true;
                s.planCs = 0.5f;
                s.planLo = {-1.0f, 0.0f, -1.0f};
                s.planHi = {1.0f, 1.0f, 1.0f};
                float cs = 0.5f;
                std::unique_ptr<PsVec3f> lo(new PsVec3f(s.planLo)), hi(new PsVec3f(s.planHi));
                uint32_t total = 24;
                if (state == "cs") cs = 0.25f;
                if (state == "bbox") hi->x = 1.5f;
                if (state == "negzero") lo->y = -0.0f;  // equal as floats, not as bytes
                if (state == "unplanned") s.planned = false;
                if (state == "nobounds") s.bounds.clear();
                if (state == "boundsN") total = 25;
                bool finishFirst = false;
                const char* action = "";
                decide(s, cs, *lo, *hi, total, pending != 0, &finishFirst, &action);
                std::printf("decide %s %s pending=%d: finishFirst=%d %s\n", modes[mode], st, pending, (int)finishFirst, action);
            }
}

PsMeshInfo part(uint32_t mpus, uint32_t v, uint32_t t, int32_t overflow = -1, uint32_t flags = 0) {
    PsMeshInfo I;
    memset(&I, 0, sizeof(I));
    I.ctMPUs = mpus;
    I.ctPassedPrecheck = mpus / 2 + 1;
    I.ctSurfaceMPUs = mpus / 3;
    I.ctVertices = v;
    I.ctTriangles = t;
    I.firstOverflowMPU = overflow;
    I.ctFieldMPUs = mpus / 2;
    I.ctLaneEvals = 8ull * mpus + 512ull * I.ctFieldMPUs + 8ull * v;
    I.launchFlags = flags;
    return I;
}

void place_case(const char* name, const std::vector<PsMeshInfo>& in) {
    const size_t n = in.size();
    std::unique_ptr<PsMeshInfo[]> info(new PsMeshInfo[n]);
    std::unique_ptr<uint32_t[]> vBase(new uint32_t[n]), tBase(new uint32_t[n]);
    std::unique_ptr<PsMeshInfo> T(new PsMeshInfo);
    for (size_t p = 0; p < n; ++p) info[p] = in[p];
    int rc = place(info.get(), n, vBase.get(), tBase.get(), T.get());
    std::printf("place %s: rc=%d", name, rc);
    if (rc == PSGPU_RET_SUCCESS) {
        for (size_t p = 0; p < n; ++p) std::printf(" [%u %u]", vBase[p], tBase[p]);
        print_info(*T);
    }
    std::printf("\n");
    // the same counts as k_finish words through the multi-process path (no launch flags there)
    std::unique_ptr<uint32_t[]> words(new uint32_t[8 * n]);
    for (size_t p = 0; p < n; ++p) {
        const PsMeshInfo& I = in[p];
        const uint32_t w[8] = {I.ctMPUs, I.ctVertices, I.ctTriangles, I.ctPassedPrecheck, I.ctSurfaceMPUs, I.ctFieldMPUs,
                               I.firstOverflowMPU < 0 ? 0x7fffffffu : (uint32_t)I.firstOverflowMPU, 0u};
        memcpy(words.get() + 8 * p, w, sizeof(w));
    }
    std::unique_ptr<PsGroupPart[]> parts(new PsGroupPart[n]);
    rc = place_words(words.get(), (int)n, parts.get(), T.get());
    std::printf("place_words %s: rc=%d", name, rc);
    if (rc == PSGPU_RET_SUCCESS) {
        print_info(*T);
        std::printf("\n");
        for (size_t p = 0; p < n; ++p) {
            const PsGroupPart& P = parts[p];
            std::printf("  rank %zu: device=%d mpus=[%u %u) bases=[%u %u] reserved=%u", p, P.device, P.mpuBegin, P.mpuEnd,
                        P.vertexBase, P.triangleBase, P.reserved);
            print_info(P.info);
            std::printf("\n");
        }
    } else {
        std::printf("\n");
    }
}

void place_cases() {
    const uint32_t big = 0xfffffff0u;
    place_case("one", {part(10, 100, 200, -1, 5)});
    place_case("all_empty", {part(0, 0, 0), part(0, 0, 0), part(0, 0, 0)});
    place_case("empty_between", {part(4, 30, 50), part(0, 0, 0), part(6, 70, 90)});
    place_case("v_max", {part(1, big, 1), part(1, 15, 1)});  // 2^32 - 1 vertices fit
    place_case("v_over", {part(1, big, 1), part(1, 16, 1)});
    place_case("t_max", {part(1, 1, big), part(1, 1, 10), part(1, 1, 5)});
    place_case("t_over", {part(1, 1, big), part(1, 1, 10), part(1, 1, 6)});
    place_case("overflow_last", {part(4, 10, 10), part(4, 10, 10), part(4, 10, 10, 9)});
    place_case("overflow_first_wins", {part(4, 10, 10), part(4, 10, 10, 6), part(4, 10, 10, 9)});
    place_case("overflow_mpu0", {part(4, 10, 10, 0), part(4, 10, 10, 6)});
    place_case("flags_or", {part(2, 3, 4, -1, 1), part(2, 3, 4, -1, 8), part(0, 0, 0, -1, 0), part(2, 3, 4, -1, 2)});
}

void decode_cases() {
    const uint32_t overflow[] = {0x7fffffffu, 0u, 5u};
    for (uint32_t ov : overflow) {
        std::unique_ptr<uint32_t[]> w(new uint32_t[8]{12u, 3000u, 5000u, 9u, 7u, 8u, ov, 0u});
        const PsMeshInfo I = decode(w.get());
        std::printf("decode overflow=%u:", ov);
        print_info(I);
        std::printf("\n");
        // psgpu_finish's own formula (psgpu_plan.h mesh_info) for a run of the same counts
        std::unique_ptr<psgpu::DevCounters> h(new psgpu::DevCounters);
        memset(h.get(), 0, sizeof(psgpu::DevCounters));
        h->firstOverflow = (int32_t)ov;
        h->shard[0].p = w[5] - 1;
        h->shard[63].p = 1;
        h->shard[1].b = w[3] - w[5];
        h->shard[2].v = w[1] - 1000;
        h->shard[7].v = 1000;
        h->shard[3].t = w[2];
        h->shard[4].s = w[4];
        const PsMeshInfo M = psgpu::mesh_info(*h, psgpu::LaunchPlan{}, w[0], false);
        EXPECT(M.ctLaneEvals == I.ctLaneEvals);
        EXPECT(!memcmp(&M, &I, sizeof(PsMeshInfo)));  // (launchFlags 0: a plain plan, no re-run)
    }
}

}  // namespace

int main() {
    even_cases();
    decide_cases();
    place_cases();
    decode_cases();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
