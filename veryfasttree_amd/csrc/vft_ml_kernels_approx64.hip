// The double instances of the two line-search kernels with -approxml's branch of the posteriors compiled in (vft_kernels_ml.h,
// VFT_ML_APPROX_INSTANCES): a translation unit of its own, like the exact instances' units.
#include <hip/hip_runtime.h>
#include <cstdint>

#include "vft_layout.h"
#include "vft_device.h"
#include "vft_kernels_profile.h"
#include "vft_kernels_ml.h"

VFT_ML_APPROX_INSTANCES(, double)
