// The grouped weight-gradient launch (wgrad_group_kernel), part 8 (see the end of mfma_dispatch.h).
#define ARL_CONV_PART 8
#include "mfma_conv_impl.h"
