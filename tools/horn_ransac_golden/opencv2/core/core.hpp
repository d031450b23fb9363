// tools/horn_ransac_golden/opencv2/core/core.hpp — TEST INFRASTRUCTURE: what src/Sim3Solver.cc includes; see ../../horn_cv.hpp
#include "../../horn_cv.hpp"
