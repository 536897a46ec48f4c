// The bf16x3 split-precision instantiations (element tag f32x3, policy key 53) of conv.hip's igemm_kernel
// and wgrad_kernel, with their launchers igemm_x3_launch / wgrad_x3_launch. A translation unit of its own
// so that the build compiles them beside conv.hip's exact fp32 and bf16 instantiations, not after them.
#define ARGUS_CONV_X3_TU 1
#include "conv.hip"
