// tests/adapter_shim/adapter_sim3_opt_main.cpp — TEST INFRASTRUCTURE.  Optimizer::OptimizeSim3 of include/planar_adapters.hpp (PLANAR_ADAPTERS_WITH_SIM3_OPT) executed
// through the reference's signature on stand-in key frames and map points that hold what the adapter reads.  Same input as the fixture generator's driver
// (tools/sim3_opt_golden/ref_sim3_opt_main.cpp; written by tests/sim3_opt_cases.py) and the same output blocks, so the result is compared with
// tests/golden/sim3_opt_ref.npz.
//   adapter_sim3_opt <in.bin> <out.bin>
#include "sim3_pair_standins.hpp"
#include "g2o_sim3_standin.hpp"

namespace Planar_SLAM {
class Optimizer {
public:
    int static OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2, const bool bFixScale);
};
}  // namespace Planar_SLAM

#define PLANAR_ADAPTERS_WITH_SIM3_OPT
#include "planar_adapters.hpp"

using namespace Planar_SLAM;
using namespace adapter_io;

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    Blocks bl;
    if (!bl.load(argv[1]) || bl.size() != 14) { std::fprintf(stderr, "cannot read 14 blocks from %s\n", argv[1]); return 2; }
    const double* prm = (const double*)bl[0].data();
    Side s1, s2;
    s1.load(bl, 1); s2.load(bl, 7);
    const int32_t* m_in = (const int32_t*)bl[13].data();
    const int n1 = (int)(bl[13].size() / 4);
    if (n1 != s1.n) return 2;
    std::vector<MapPoint> foreign;
    std::vector<MapPoint*> vpMatches1 = s1.matches(m_in, s2, foreign);
    g2o::Sim3 S12;
    for (int k = 0; k < 8; k++) S12[k] = prm[2 + k];
    const int nIn = Optimizer::OptimizeSim3(&s1.kf, &s2.kf, vpMatches1, S12, (float)prm[0], prm[1] != 0.0);
    std::vector<int32_t> m_out(m_in, m_in + n1);
    for (int i = 0; i < n1; i++) if (!vpMatches1[i]) m_out[i] = -1;
    double So[8];
    for (int k = 0; k < 8; k++) So[k] = S12[k];
    FILE* f = std::fopen(argv[2], "wb");
    if (!f) return 2;
    write_block(f, m_out.data(), m_out.size()); write_block(f, &nIn, 1); write_block(f, So, 8);
    std::fclose(f);
    return 0;
}
