// tools/horn_ransac_golden/opencv2/opencv.hpp — TEST INFRASTRUCTURE: what include/Sim3Solver.h includes; see ../horn_cv.hpp
#include "../horn_cv.hpp"
