// filter_check.cpp — psgpu::SimdPolyGpu::weldFilter() compiled as a host would compile it
// (tests/test_gpu_filter.py).
//
//   filter_check <soa.bin> <cellsize> <out.bin>
//
// soa.bin: SOABlobPrims | SOABlobPrimMatrices | SOABlobOps bytes.  Runs the model, welds the
// finished run, asks for its shells, filters with the all-zero filter and writes rc of
// weldFilter before the shells, rc of setModel / run / finish / weld / weldShells / weldFilter /
// weldFilterDevice, then pos, nrm, col, tris, vertexMap, shellMap and the PsShell records.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "parsip_gpu.hpp"

template <class T>
static void put(std::ofstream& o, const std::vector<T>& v) {
    o.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

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
    Poly::Shells sh;
    Poly::Filtered f;
    int32_t rc[8];
    rc[1] = poly.setModel(prims, mats, ops);
    rc[2] = poly.run((float)std::atof(argv[2]));
    PsMeshInfo info;
    rc[3] = poly.finish(&info);
    rc[4] = poly.weld(&w);
    rc[0] = poly.weldFilter(&f);  // a weld, no shells yet
    rc[5] = poly.weldShells(&sh);
    const PsShellFilter all{};
    rc[6] = poly.weldFilter(&f, &all);
    PsFilterDevice dev;
    rc[7] = poly.weldFilterDevice(&dev);
    if (rc[7] == PSGPU_RET_SUCCESS && !(dev.pos && dev.nrm && dev.col && dev.tris && dev.vertexMap && dev.shellMap && dev.shells))
        rc[7] = -1;
    std::printf("weldFilter rc %d: %u of %u shells, %u of %u vertices, %u of %u triangles\n", rc[6], f.info.ctShells,
                f.info.ctInputShells, f.info.ctVertices, f.info.ctInputVertices, f.info.ctTriangles,
                f.info.ctInputTriangles);
    std::ofstream o(argv[3], std::ios::binary);
    o.write(reinterpret_cast<const char*>(rc), sizeof rc);
    put(o, f.pos);
    put(o, f.nrm);
    put(o, f.col);
    put(o, f.tris);
    put(o, f.vertexMap);
    put(o, f.shellMap);
    put(o, f.shells);
    return o ? 0 : 66;
}
