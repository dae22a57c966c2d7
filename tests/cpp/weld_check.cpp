// weld_check.cpp — psgpu::SimdPolyGpu::weld() compiled as a host would compile it
// (tests/test_gpu_weld.py).
//
//   weld_check <soa.bin> <cellsize> <out.bin>
//
// soa.bin: SOABlobPrims | SOABlobPrimMatrices | SOABlobOps bytes.  Runs the model, welds the
// finished run and writes rc of weld before any run, rc of run / finish / weld, the four
// PsWeldInfo counts, then pos | nrm | col | tris | vertexMap.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "parsip_gpu.hpp"

int main(int argc, char** argv) {
    if (argc < 4) return 64;
    static PsSoaBlobPrims prims;
    static PsSoaPrimMatrices mats;
    static PsSoaBlobOps ops;
    std::ifstream in(argv[1], std::ios::binary);
    in.read(reinterpret_cast<char*>(&prims), sizeof prims);
    in.read(reinterpret_cast<char*>(&mats), sizeof mats);
    in.read(reinterpret_cast<char*>(&ops), sizeof ops);
    if (!in) return 65;
    using Poly = psgpu::SimdPolyGpu<PsSoaBlobPrims, PsSoaPrimMatrices, PsSoaBlobOps>;
    Poly poly(0);
    Poly::Welded w;
    int32_t rc[5];
    rc[0] = poly.weld(&w);  // no finished run yet
    rc[1] = poly.setModel(prims, mats, ops);
    rc[2] = poly.run((float)std::atof(argv[2]));
    PsMeshInfo info;
    rc[3] = poly.finish(&info);
    rc[4] = poly.weld(&w);
    std::printf("weld rc %d: %u -> %u vertices, %u triangles\n", rc[4], w.info.ctInputVertices, w.info.ctVertices,
                w.info.ctTriangles);
    std::ofstream o(argv[3], std::ios::binary);
    o.write(reinterpret_cast<const char*>(rc), sizeof rc);
    const uint32_t counts[6] = {w.info.ctVertices, w.info.ctTriangles, w.info.ctInputVertices, w.info.ctSeamVertices,
                                info.ctVertices, info.ctTriangles};
    o.write(reinterpret_cast<const char*>(counts), sizeof counts);
    o.write(reinterpret_cast<const char*>(w.pos.data()), (std::streamsize)(w.pos.size() * 4));
    o.write(reinterpret_cast<const char*>(w.nrm.data()), (std::streamsize)(w.nrm.size() * 4));
    o.write(reinterpret_cast<const char*>(w.col.data()), (std::streamsize)(w.col.size() * 4));
    o.write(reinterpret_cast<const char*>(w.tris.data()), (std::streamsize)(w.tris.size() * 4));
    o.write(reinterpret_cast<const char*>(w.vertexMap.data()), (std::streamsize)(w.vertexMap.size() * 4));
    return o ? 0 : 66;
}
