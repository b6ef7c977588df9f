// Element math of the LeakyReLU kernels (leaky.hip) and of their host-pointer twins (leaky_twins.hip): one definition compiled for both
// sides, so a twin returns the device's bits.  RNDModel's predictor and target (cleanrl/ppo_rnd_envpool.py:188-233) put nn.LeakyReLU()
// behind each of their three convolutions; every forward kernel here fuses a ReLU, so these two sit behind a pre-activation forward
// (kernel Z's Z_BIAS epilogue) and behind a data gradient called with an all-ones mask.
//
// Forward, as torch defines it (one f32 multiply, the slope rounded to f32 once):  a = z > 0 ? z : z * slope.  -0 stays -0, a NaN stays a NaN.
// Backward:  dz = bit ? da : da * slope  with bit = (z > 0), the forward's mask bit.
// Mask bits: word w, bit b <-> flat element 32 w + b (the layout of the *_bits forwards); (n + 31) / 32 words, the bits past n zero.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace mi355ppo {

MI355_HD float leaky_fwd(float z, float slope) { return z > 0.0f ? z : z * slope; }
MI355_HD float leaky_bwd(float da, bool bit, float slope) { return bit ? da : da * slope; }

}  // namespace mi355ppo
