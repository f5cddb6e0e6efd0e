// dqp_al_banded_launch.h -- the launch rule of the narrow block-tridiagonal Newton kernel (knots of up to 16 variables),
// for the files that instantiate it: dqp_al_banded.hip (registered models, Given<> with control bounds) and
// dqp_al_banded_box.hip (Given<> with a state box).
#ifndef DQP_AL_BANDED_LAUNCH_H_
#define DQP_AL_BANDED_LAUNCH_H_
#include "dqp_al_banded_kernels.h"
#include "dqp_trace.h"

#ifndef BAND_STAMP_ARG      // the instrumented build of dqp_al_banded.hip passes its stamp buffer
#define BAND_STAMP_ARG
#endif

namespace {

// Eight problems per wavefront where a knot fits a half row AND the batch is more than one wavefront per SIMD at
// four per wavefront (these kernels hold one wavefront per SIMD): below that the launch is one latency chain per
// wavefront either way and the narrower group only idles SIMDs (cartpole-1 at B = 4096: 2.0 ms both ways;
// cartpole-2 at B = 8192: 2.24 -> 1.97 ms per AL_mpc.MPC call).  dqp::al_banded_narrow(B) decides (dqp_al_banded.hip).
template <class Map> constexpr bool half_row() { return Map::NX + Map::NU <= 8; }
template <class Map> int run_newton(const BandP &P, void *stream)
{
    if constexpr (half_row<Map>()) {
        if (dqp::al_banded_narrow(P.B)) {
            if constexpr (Map::NX + Map::NU >= 6) {
                // the one-wavefront-per-SIMD half-row models: the factor stays in LDS where the horizon allows (four
                // workgroups per CU next to their 5 KB tiles)
                using C = BandCfg<Map>;
                const size_t bytes = (size_t)P.T * (C::ROW + 1) * 8 * C::NT * sizeof(double);
                if (bytes <= 34 * 1024) {
                    DQP_LAUNCH((al_banded_newton_kernel<Map, 8, true>), dim3((P.B + 7) / 8), dim3(64), bytes, (hipStream_t)stream, P BAND_STAMP_ARG);
                    return dqp::launched();
                }
            }
            DQP_LAUNCH((al_banded_newton_kernel<Map, 8>), dim3((P.B + 7) / 8), dim3(64), 0, (hipStream_t)stream, P BAND_STAMP_ARG);
            return dqp::launched();
        }
    }
    DQP_LAUNCH((al_banded_newton_kernel<Map, 16>), dim3((P.B + 3) / 4), dim3(64), 0, (hipStream_t)stream, P BAND_STAMP_ARG);
    return dqp::launched();
}

}  // namespace
#endif
