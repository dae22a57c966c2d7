// shells_check.cpp — psgpu::SimdPolyGpu::weldShells() compiled as a host would compile it
// (tests/test_gpu_shells.py).
//
//   shells_check <soa.bin> <cellsize> <out.bin>
//
// soa.bin: SOABlobPrims | SOABlobPrimMatrices | SOABlobOps bytes.  Runs the model, welds the
// finished run, asks for its shells and writes rc of weldShells before the weld, rc of
// setModel / run / finish / weld / weldShells / weldShellsDevice, then the PsShell records,
// the PsShellsInfo, vertexShell and triShell.
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
    Poly::Shells sh;
    int32_t rc[7];
    rc[1] = poly.setModel(prims, mats, ops);
    rc[2] = poly.run((float)std::atof(argv[2]));
    PsMeshInfo info;
    rc[3] = poly.finish(&info);
    rc[0] = poly.weldShells(&sh);  // a finished run, no weld yet
    rc[4] = poly.weld(&w);
    rc[5] = poly.weldShells(&sh);
    PsShellsDevice dev;
    rc[6] = poly.weldShellsDevice(&dev);
    if (rc[6] == PSGPU_RET_SUCCESS && !(dev.shells && dev.vertexShell && dev.triShell)) rc[6] = -1;
    std::printf("weldShells rc %d: %u shells, %u closed, area %.17g, volume %.17g\n", rc[5], sh.info.ctShells,
                sh.info.ctClosedShells, sh.info.area, sh.info.volume);
    std::ofstream o(argv[3], std::ios::binary);
    o.write(reinterpret_cast<const char*>(rc), sizeof rc);
    o.write(reinterpret_cast<const char*>(sh.shells.data()), (std::streamsize)(sh.shells.size() * sizeof(PsShell)));
    o.write(reinterpret_cast<const char*>(&sh.info), sizeof sh.info);
    o.write(reinterpret_cast<const char*>(sh.vertexShell.data()), (std::streamsize)(sh.vertexShell.size() * 4));
    o.write(reinterpret_cast<const char*>(sh.triShell.data()), (std::streamsize)(sh.triShell.size() * 4));
    return o ? 0 : 66;
}
