// tools/pnp_ransac_golden/opencv2/core/core.hpp — TEST INFRASTRUCTURE: what the reference's #include <opencv2/core/core.hpp> finds in the PnPsolver golden build
#pragma once
#include "../../pnp_cv.hpp"
