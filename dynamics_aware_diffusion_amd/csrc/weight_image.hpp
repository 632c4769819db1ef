// weight_image.hpp — the layout of the packed weight images the conv-GEMM kernels read, in one place:
// dad_model_finalize packs them on the host (host_plan.hpp pack_image), dad_model_refresh_weights rebuilds
// them on the device (train_bwd.hpp repack_many_kernel).  No HIP dependency (tests/sanitize/ builds it host-only).
//   image index = (((ci / kg) * wtaps + slot) * M + o) * kg + ci % kg
#pragma once
#include <stdint.h>

#include "conv_shapes.hpp"

namespace dad {

enum ImageMode {
    IMG_FWD = 0,        // Conv1d (co, ci, K) [+ riding 1x1 conv as slot K]
    IMG_FWD_UP = 1,     // ConvTranspose1d (ci, co, 4) as two 2-tap phases, M = 2 co
    IMG_BWD_CONV = 2,   // data gradient of Conv1d: (m, c, K-1-slot) <- W[c][c_lo + m][.]
    IMG_BWD_DOWN = 3,   // data gradient of Downsample1d as a transposed conv whose 4th tap is zero
    IMG_BWD_UP = 4,     // data gradient of Upsample1d as a 5-tap stride-2 conv whose first tap is zero
    IMG_BWD_FINAL = 5,  // data gradient of final_conv[1]
};
struct ImageDesc {
    float* dst; const float* w; const float* ride;     // ride: the 1x1 residual conv's weight, or nullptr
    long n;                                            // elements of the image
    int32_t mode, kg, wtaps, M;
    int32_t CO, CI, K;                                 // the SOURCE tensor's dims as the mode reads them
    int32_t c_lo, c_n;                                 // IMG_BWD_CONV: input-channel range of the forward conv
};

// Element (input channel ci, tap slot, output column o) of the image; zero in the padding.
DAD_HD inline float image_value(const ImageDesc& p, int ci, int slot, int o) {
    switch (p.mode) {
        case IMG_FWD:
            if (ci < p.CI) {
                if (slot < p.K) return p.w[((long)o * p.CI + ci) * p.K + slot];
                if (p.ride != nullptr) return p.ride[(long)o * p.CI + ci];
            }
            break;
        case IMG_FWD_UP: case IMG_BWD_DOWN: {
            // y[co, 2j] = W[.,co,3] x[j-1] + W[.,co,1] x[j]: columns [0, co); y[co, 2j+1] = W[.,co,2] x[j] + W[.,co,0] x[j+1]
            const int co = p.M >> 1, half = o >= co, oo = o - half * co;
            const int kk = half == 0 ? (slot == 0 ? 3 : 1) : (slot == 0 ? 2 : 0);
            if (p.mode == IMG_FWD_UP) { if (ci < p.CI) return p.w[((long)ci * co + oo) * 4 + kk]; }
            else if (ci < p.CO && kk < 3) return p.w[((long)ci * p.CI + oo) * 3 + kk];       // W (co_f = ci, ci_f = oo, k)
            break;
        }
        case IMG_BWD_CONV:
            if (o < p.c_n && ci < p.CO) return p.w[((long)ci * p.CI + p.c_lo + o) * p.K + (p.K - 1 - slot)];
            break;
        case IMG_BWD_UP:
            if (slot >= 1 && o < p.CI && ci < p.CO) return p.w[((long)o * p.CO + ci) * 4 + (slot - 1)];   // Wt (ci_f = o, co_f = ci, kk)
            break;
        case IMG_BWD_FINAL:
            if (ci < p.CO) return p.w[(long)ci * p.CI + o];                                      // Wf (td = ci, dim = o)
            break;
    }
    return 0.0f;
}

}  // namespace dad
