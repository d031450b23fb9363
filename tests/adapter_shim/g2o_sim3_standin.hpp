// tests/adapter_shim/g2o_sim3_standin.hpp — TEST INFRASTRUCTURE: the part of g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h) the OptimizeSim3 adapter touches, for
// builds without the reference tree: eight doubles behind operator[], quaternion x, y, z, w, then t, then s.
#pragma once
namespace g2o {
struct Sim3 {
    double r[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1;
    double operator[](int i) const { return i < 4 ? r[i] : i < 7 ? t[i - 4] : s; }
    double& operator[](int i) { return i < 4 ? r[i] : i < 7 ? t[i - 4] : s; }
};
}  // namespace g2o
