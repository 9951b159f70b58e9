// value_net_lstm_worlds.hip -- LSTM-RL's float32 decision (value_net_lstm.hip: cs_value_net_decide_lstm) from the resident worlds
// (cs_value_net_decide_lstm_worlds; Python: LstmRL.set_recurrent_input("fused")): the kernel generates a step's rows in LDS, and rotated
// [W][A][n][13|15] -- 431 MB at 4096 worlds x 81 actions x 25 humans -- is neither allocated, written nor gathered back.  Replaces
// cs_lookahead + cs_value_net_decide_lstm, whose results it reproduces bit for bit.  The kernel is value_net_lstm_body.inc under LSTM_OM 0
// with the three seams of value_net_lstm_worlds.h; the LDS map, the blob and the (WREG, MLP1) choice are k_value_net_lstm's, the frame table
// lies behind the map.  This file is the kernel's name and the entry.
#include <hip/hip_runtime.h>

#include "value_net_lstm_f32.h"
#include "value_net_lstm_worlds.h"

namespace {

template <bool WREG, bool MLP1>
__global__ __launch_bounds__(NT) void k_value_net_lstm_worlds(LstmPlan q, LstmLds m, const float* __restrict__ wb, int NG, int A, int n, int sorted,
                                                              LstmWorlds world, const float* __restrict__ robot, int rstride, float gamma, float dt,
                                                              float* __restrict__ values)
{
#define LSTM_OM 0
#include "value_net_lstm_body.inc"
#undef LSTM_OM
}

} // namespace

#include "value_net_pick.h"

extern "C" int cs_value_net_decide_lstm_worlds(const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n,
                                               int theta_and_omega_visible, int sorted_by_distance, const float* d_actions, const float* d_next,
                                               const float* d_current, const float* d_robot, int robot_stride, float gamma, float dt,
                                               const int32_t* d_override, float* d_rewards_out, float* d_values, int32_t* d_choice, float* d_action_out,
                                               void* stream)
{
    LstmPlan q;
    const int rc = build_lstm_plan(dims, n_dims, theta_and_omega_visible ? 15 : 13, q);
    if (rc != CS_OK) return rc;
    // (the worlds' two arrays stand where cs_value_net_decide_lstm has cs_lookahead's two outputs: cs_lookahead's own checks are among these)
    const int rc2 = lstm_check_decide("cs_value_net_decide_lstm_worlds", q.v, d_weights, n_weight_floats, W, A, n, sorted_by_distance, d_next, d_current,
                                      d_actions, d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    const LstmLds m = lstm_lds_map(q, n);
    const LstmWorlds world{d_actions, d_next, d_current, d_rewards_out, m.total, theta_and_omega_visible ? 1 : 0};      // (the frame table: behind the map)
    const bool wreg = q.g.ncb <= 4 * RB && q.g.kg_total <= RKG, mlp1 = q.v.c0[1] > 0;
    const int rc3 = lstm_launch(m.total + JROWS * LA_FRAME_FLOATS, W, A, wreg, mlp1, [&](auto WR, auto M1, size_t shmem, int NG, int grid) {
        constexpr auto kernel = k_value_net_lstm_worlds<decltype(WR)::value, decltype(M1)::value>;
        const int rc4 = grant_lds<kernel>(shmem);
        if (rc4 != CS_OK) return rc4;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), shmem, (hipStream_t)stream, q, m, d_weights, NG, A, n, sorted_by_distance, world, d_robot,
                           robot_stride, gamma, dt, d_values);
        return (int)CS_OK;
    });
    if (rc3 != CS_OK) return rc3;
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}
