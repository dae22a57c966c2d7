// mctables_check.cpp — the packed marching-cubes tables k_mpu's S3-S6 passes read
// (psgpu::CubeTablesDev, built by cube_tables / fill_device_tables: psgpu_model.h) compiled as
// plain host C++ and checked, entry by entry, against a naive derivation from the triangle table
// alone, for tests/test_mcsweep.py.
//
//   mctables_check <tritable.bin>
//
// tritable.bin: int32[256][16], the triangle table (-1 ends a row) of the CPU oracle
//               (psor_tritable), which the library's own (psgpu_tritable) must equal.
// stdout: one line "configs C own_pairs P kth_edges K cell_edges E failures F".  The first few
// failures are described on stderr; the exit code is 1 if there was one.
//
// The naive side knows the edges by their names only (the reference's numbering LB LT LN LF RB RT
// RN RF BN BF TN TF: the two faces an edge lies in, L / R: x = 0 / 1, B / T: y = 0 / 1, N / F:
// z = 0 / 1) and cells by their coordinates: an edge's vertex is new in the first cell, in
// (i, j, k) order, that contains the edge.  The decodes of the packed words are restated from
// psgpu_device.h (count_cells, vertex_records, CellEdge), which compiles for the device only.
#define PSGPU_MODEL_NO_HIP
#include "psgpu_model.h"

#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

using namespace psgpu;

namespace {

int failures = 0;
void fail(const char* what, int a, int b, int c, long got, long want) {
    if (failures++ < 10) fprintf(stderr, "%s at (%d, %d, %d): got %ld, want %ld\n", what, a, b, c, got, want);
}

struct NaiveEdge {
    int lo[3];  // the edge's low corner, in cell-corner coordinates 0 / 1
    int ax;     // the axis it runs along
};

// the (corner, axis) of an edge from its name
NaiveEdge edge_of(const char* name) {
    int fixed[3] = {-1, -1, -1};
    for (int q = 0; q < 2; ++q) switch (name[q]) {
        case 'L': fixed[0] = 0; break;
        case 'R': fixed[0] = 1; break;
        case 'B': fixed[1] = 0; break;
        case 'T': fixed[1] = 1; break;
        case 'N': fixed[2] = 0; break;
        case 'F': fixed[2] = 1; break;
        }
    NaiveEdge e{};
    for (int a = 0; a < 3; ++a) {
        if (fixed[a] < 0) e.ax = a;
        e.lo[a] = fixed[a] < 0 ? 0 : fixed[a];
    }
    return e;
}

const char* const kNames[12] = {"LB", "LT", "LN", "LF", "RB", "RT", "RN", "RF", "BN", "BF", "TN", "TF"};

// the device's decode of CubeTablesDev::edge (CellEdge, psgpu_device.h)
struct Slot {
    int sx, sy, sz, ax;
    Slot(uint64_t edgeBits, int i, int j, int k, int ed) {
        const int eb = (int)((edgeBits >> (5 * ed)) & 31u), c1 = eb & 7;
        sx = i + ((c1 >> 2) & 1), sy = j + ((c1 >> 1) & 1), sz = k + (c1 & 1), ax = eb >> 3;
    }
    int slot() const { return ((sx * 8 + sy) * 8 + sz) * 3 + ax; }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s tritable.bin\n", argv[0]);
        return 2;
    }
    std::vector<int32_t> tri(256 * 16);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(tri.data(), 4, tri.size(), f) != tri.size()) return 3;
    fclose(f);

    const CubeTables& T = cube_tables();
    std::unique_ptr<CubeTablesDev> Dp(new CubeTablesDev);
    CubeTablesDev& D = *Dp;
    fill_device_tables(T, D);

    NaiveEdge E[12];
    for (int e = 0; e < 12; ++e) E[e] = edge_of(kNames[e]);

    // 1. per configuration: the library's table is the given one; row, order, cross, ntri
    int configs = 0;
    for (int c = 0; c < 256; ++c, ++configs) {
        std::vector<int> row, distinct;
        for (int q = 0; q < 16; ++q) {
            if (T.tri[c][q] != tri[c * 16 + q]) fail("psgpu_tritable", c, q, 0, T.tri[c][q], tri[c * 16 + q]);
            if (tri[c * 16 + q] < 0) break;
            row.push_back(tri[c * 16 + q]);
        }
        if (row.size() % 3 != 0 || row.size() > 15) fail("row length", c, 0, 0, (long)row.size(), 0);
        for (int e : row) {
            bool seen = false;
            for (int d : distinct) seen |= d == e;
            if (!seen) distinct.push_back(e);
        }
        // the sign-changing edges, from the configuration's bits and the edges' names
        uint32_t cross = 0;
        for (int e = 0; e < 12; ++e) {
            const int c1 = E[e].lo[0] * 4 + E[e].lo[1] * 2 + E[e].lo[2], c2 = c1 + (4 >> E[e].ax);
            if (((c >> c1) & 1) != ((c >> c2) & 1)) cross |= 1u << e;
        }
        uint32_t used = 0;
        for (int e : distinct) used |= 1u << e;
        if (used != cross) fail("row's edge set against the crossing edges", c, 0, 0, used, cross);
        if (D.cross[c] != cross) fail("cross", c, 0, 0, D.cross[c], cross);
        if (D.ntri[c] != row.size() / 3) fail("ntri", c, 0, 0, D.ntri[c], (long)row.size() / 3);
        if ((D.crossNtri[c] & 0xffffu) != cross || (D.crossNtri[c] >> 16) != row.size() / 3)
            fail("crossNtri", c, 0, 0, D.crossNtri[c], cross | (row.size() / 3) << 16);
        for (int q = 0; q < 16; ++q) {
            const long got = (long)((D.row[c] >> (4 * q)) & 15u), want = q < (int)row.size() ? row[q] : 0;
            if (got != want) fail("row", c, q, 0, got, want);
            const long gotO = (long)((D.order[c] >> (4 * q)) & 15u), wantO = q < (int)distinct.size() ? distinct[q] : 0;
            if (gotO != wantO) fail("order", c, q, 0, gotO, wantO);
        }
    }

    // 2. per (configuration, ownership class): new vertices, triangles, and the k-th owned edge.
    // A cell of class b sits at coordinate 0 along the axes whose bit is set and at 1 along the
    // others; the cells that contain an edge are its own and, along each off-axis direction in
    // which the edge lies on the cell's low face, the neighbour below (if the lattice has one).
    int pairs = 0, kth = 0;
    for (int b = 0; b < 8; ++b) {
        const int at[3] = {(b & 4) ? 0 : 1, (b & 2) ? 0 : 1, (b & 1) ? 0 : 1};
        bool owned[12];
        for (int e = 0; e < 12; ++e) {
            owned[e] = true;
            for (int a = 0; a < 3; ++a)
                if (a != E[e].ax && E[e].lo[a] == 0 && at[a] > 0) owned[e] = false;  // the cell below has it first
        }
        uint32_t ownMask = 0;
        for (int e = 0; e < 12; ++e) ownMask |= owned[e] ? 1u << e : 0u;
        if (D.own[b] != ownMask) fail("own", b, 0, 0, D.own[b], ownMask);
        for (int c = 0; c < 256; ++c, ++pairs) {
            std::vector<int> mine;  // the row's owned edges in first-occurrence order
            int nt = 0;
            for (int q = 0; q < 16 && tri[c * 16 + q] >= 0; ++q) {
                const int e = tri[c * 16 + q];
                nt += q % 3 == 2;
                bool seen = false;
                for (int d : mine) seen |= d == e;
                if (!seen && owned[e]) mine.push_back(e);
            }
            // count_cells: one lookup, popcount of the owned crossing edges | triangles << 16
            const uint32_t cn = D.crossNtri[c];
            const uint32_t nvt = (uint32_t)__builtin_popcount(D.own[b] & cn & 0xfffu) | (cn & 0xffff0000u);
            if ((nvt & 0xffffu) != mine.size()) fail("new vertices", c, b, 0, nvt & 0xffffu, (long)mine.size());
            if ((int)(nvt >> 16) != nt) fail("triangles", c, b, 0, nvt >> 16, nt);
            // vertex_records: the (left + 1)-th owned edge of the row order
            for (uint32_t k = 0; k < mine.size(); ++k, ++kth) {
                uint32_t left = k;
                int ed = 0;
                for (int q = 0; q < 12; ++q) {
                    ed = (int)((D.order[c] >> (4 * q)) & 15u);
                    if ((D.own[b] >> ed) & 1u) {
                        if (left == 0u) break;
                        --left;
                    }
                }
                if (ed != mine[k]) fail("k-th owned edge", c, b, (int)k, ed, mine[k]);
            }
        }
    }

    // 3. CellEdge: every edge of every cell against its named (corner, axis); cells that share
    // a lattice edge name it by one slot, and no two lattice edges share a slot
    int cellEdges = 0;
    std::map<std::vector<int>, int> slotOf;  // the edge's two end corners in the 8^3 cache -> slot
    std::map<int, std::vector<int>> edgeOf;
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j < 7; ++j)
            for (int k = 0; k < 7; ++k)
                for (int e = 0; e < 12; ++e, ++cellEdges) {
                    const Slot s(D.edge, i, j, k, e);
                    const int lo[3] = {i + E[e].lo[0], j + E[e].lo[1], k + E[e].lo[2]};
                    if (s.sx != lo[0] || s.sy != lo[1] || s.sz != lo[2] || s.ax != E[e].ax)
                        fail("CellEdge", i * 49 + j * 7 + k, e, 0, s.slot(), ((lo[0] * 8 + lo[1]) * 8 + lo[2]) * 3 + E[e].ax);
                    if (s.slot() < 0 || s.slot() >= 1536) fail("slot range", i * 49 + j * 7 + k, e, 0, s.slot(), 1535);
                    // the oracle's corner1 / corner2 of the same edge, through the library's table
                    int hi[3] = {lo[0], lo[1], lo[2]};
                    hi[E[e].ax] += 1;
                    const int c1 = T.corner1[e], c2 = T.corner2[e];
                    const int a1[3] = {i + ((c1 >> 2) & 1), j + ((c1 >> 1) & 1), k + (c1 & 1)};
                    const int a2[3] = {i + ((c2 >> 2) & 1), j + ((c2 >> 1) & 1), k + (c2 & 1)};
                    if (memcmp(a1, lo, sizeof lo) != 0 || memcmp(a2, hi, sizeof hi) != 0 || T.axis[e] != E[e].ax)
                        fail("corner1 / corner2 / axis", e, 0, 0, c1 * 8 + c2, 0);
                    const std::vector<int> key = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
                    auto it = slotOf.find(key);
                    if (it == slotOf.end()) slotOf[key] = s.slot();
                    else if (it->second != s.slot()) fail("shared edge, two slots", i * 49 + j * 7 + k, e, 0, s.slot(), it->second);
                    auto jt = edgeOf.find(s.slot());
                    if (jt == edgeOf.end()) edgeOf[s.slot()] = key;
                    else if (jt->second != key) fail("two edges, one slot", i * 49 + j * 7 + k, e, 0, s.slot(), -1);
                }
    if (slotOf.size() != 3 * 7 * 8 * 8) fail("lattice edges of an MPU", 0, 0, 0, (long)slotOf.size(), 3 * 7 * 8 * 8);

    printf("configs %d own_pairs %d kth_edges %d cell_edges %d failures %d\n", configs, pairs, kth, cellEdges, failures);
    return failures ? 1 : 0;
}
