// group_weld_check.cpp — psgpu::SimdPolyT::weld() compiled as a host would compile it, over the
// mock BlobTree (tests/test_gpu_group_weld.py).
//
//   group_weld_check <tree.txt> <cellsize> <out.bin>
//
// tree.txt: the pre-order tree file of tests/test_cpp_simdpoly.py (skeletal primitives and
// operators without parameters are enough here).  SimdPoly runs as a Group of two parts;
// PSGPU_GROUP_OPT_MIN_PART_MPUS is set to 0 so that a small lattice really runs as two.
// Writes rc of weld before any run, rc of run / weld / weldDevice, the four PsWeldInfo counts,
// the run's vertices and triangles, the number of parts and the split's middle bound, then
// pos | nrm | col | tris | vertexMap.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <vector>

#include "mock_blobtree.hpp"
#include "parsip_gpu_blobtree.hpp"

using namespace PS::BLOBTREE;

namespace {

// One node per line, pre-order (see simdpoly_check.cpp read_node)
CBlobNode* read_node(std::istream& in, std::vector<std::unique_ptr<CBlobNode>>& own) {
    int type, nk;
    in >> type >> nk;
    if (!in) return nullptr;
    float v[3 + 3 + 3 + 1 + 16 + 12 + 2];
    for (float& f : v) in >> f;
    CBlobNode* n;
    if (type >= 14) {
        n = new CBlobNode();
    } else {
        CSkeletonPrimitive* sp = new CSkeletonPrimitive();
        CSkeleton* s;
        switch (type) {
        case 0: s = new CSkeletonPoint(); break;
        case 1: s = new CSkeletonLine(); break;
        case 2: s = new CSkeletonCylinder(); break;
        case 3: s = new CSkeletonDisc(); break;
        case 4: s = new CSkeletonRing(); break;
        case 6: s = new CSkeletonCube(); break;
        case 7: s = new CSkeletonTriangle(); break;
        default: s = new CSkeleton(); break;
        }
        const float* q = v + 26;
        s->a = vec3f{q[0], q[1], q[2]};
        s->b = vec3f{q[3], q[4], q[5]};
        s->c = vec3f{q[6], q[7], q[8]};
        s->r = q[9];
        s->h = q[10];
        sp->skeleton = s;
        n = sp;
    }
    own.emplace_back(n);
    n->type = type;
    n->octree.lower = vec3f{v[0], v[1], v[2]};
    n->octree.upper = vec3f{v[3], v[4], v[5]};
    n->material.diffused = vec4f{v[6], v[7], v[8], v[38]};
    n->id = (int)v[39];
    n->transform.back.identity = v[9] != 0.0f;
    std::memcpy(n->transform.back.e, v + 10, 64);
    for (int c = 0; c < nk; ++c) n->kids.push_back(read_node(in, own));
    return n;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) return 64;
    std::ifstream in(argv[1]);
    std::vector<std::unique_ptr<CBlobNode>> own;
    CBlobNode* root = read_node(in, own);
    if (!root) return 65;
    std::unique_ptr<SimdPoly> poly(new SimdPoly(0));
    if (poly->linearizeBlobTree(root) < 0) return 66;
    if (psgpu_group_set_option(poly->group().get(), PSGPU_GROUP_OPT_MIN_PART_MPUS, 0) != PSGPU_RET_SUCCESS) return 67;
    psgpu::Welded w;
    int32_t rc[4];
    rc[0] = poly->weld(&w);  // no run yet
    rc[1] = poly->run((float)std::atof(argv[2]));
    rc[2] = poly->weld(&w);
    PsWeldDevice dev{};
    rc[3] = poly->weldDevice(&dev);
    if (rc[3] == PSGPU_RET_SUCCESS && !(dev.pos && dev.nrm && dev.col && dev.tris && dev.vertexMap)) return 68;
    std::printf("weld rc %d: %u -> %u vertices, %u triangles\n", rc[2], w.info.ctInputVertices, w.info.ctVertices,
                w.info.ctTriangles);
    const int nParts = psgpu_group_size(poly->group().get());
    std::vector<uint32_t> bounds((size_t)nParts + 1, 0u);
    if (psgpu_group_get_split(poly->group().get(), bounds.data()) != PSGPU_RET_SUCCESS) return 69;
    std::ofstream o(argv[3], std::ios::binary);
    o.write(reinterpret_cast<const char*>(rc), sizeof rc);
    const uint32_t counts[8] = {w.info.ctVertices,   w.info.ctTriangles,      w.info.ctInputVertices, w.info.ctSeamVertices,
                                poly->info().ctVertices, poly->info().ctTriangles, (uint32_t)nParts,       bounds[1]};
    o.write(reinterpret_cast<const char*>(counts), sizeof counts);
    o.write(reinterpret_cast<const char*>(w.pos.data()), (std::streamsize)(w.pos.size() * 4));
    o.write(reinterpret_cast<const char*>(w.nrm.data()), (std::streamsize)(w.nrm.size() * 4));
    o.write(reinterpret_cast<const char*>(w.col.data()), (std::streamsize)(w.col.size() * 4));
    o.write(reinterpret_cast<const char*>(w.tris.data()), (std::streamsize)(w.tris.size() * 4));
    o.write(reinterpret_cast<const char*>(w.vertexMap.data()), (std::streamsize)(w.vertexMap.size() * 4));
    return o ? 0 : 70;
}
