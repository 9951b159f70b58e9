// value_net_lstm_worlds_bf16.hip -- LSTM-RL's opt-in bf16 decision (value_net_lstm_bf16.hip: cs_value_net_decide_lstm_bf16) from the resident
// worlds (cs_value_net_decide_lstm_worlds_bf16; Python: LstmRL.set_recurrent_input("fused") beside set_recurrent_precision("bf16")).  Replaces
// cs_lookahead + cs_value_net_decide_lstm_bf16, whose results it reproduces bit for bit, on the blob of cs_value_net_pack_lstm_bf16.  The
// kernel is value_net_lstm_bf16_body.inc under LSTM_OM 0 with the three seams of value_net_lstm_worlds.h -- the generated rows are float32, as the
// gathered ones are: the arithmetic rounds nothing of a rotated column --; the plan, the LDS map and the (WREG, MLP1) choice are
// k_value_net_lstm_bf16's (value_net_lstm_bf16.h), the frame table lies behind the map.  This file is the kernel's name and the entry.
#include <hip/hip_runtime.h>

#include "value_net_lstm_bf16.h"
#include "value_net_lstm_worlds.h"

namespace {

template <bool WREG, bool MLP1>
__global__ __launch_bounds__(NT, 2) void k_value_net_lstm_worlds_bf16(LstmHPlan s, LstmHLds m, const float* __restrict__ wb, int NG, int A, int n, int sorted,
                                                                   LstmWorlds world, const float* __restrict__ robot, int rstride, float gamma, float dt,
                                                                   float* __restrict__ values)
{
#define LSTM_OM 0
#include "value_net_lstm_bf16_body.inc"
#undef LSTM_OM
}

} // namespace

#include "value_net_pick.h"

extern "C" int cs_value_net_decide_lstm_worlds_bf16(const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n,
                                                    int theta_and_omega_visible, int sorted_by_distance, const float* d_actions, const float* d_next,
                                                    const float* d_current, const float* d_robot, int robot_stride, float gamma, float dt,
                                                    const int32_t* d_override, float* d_rewards_out, float* d_values, int32_t* d_choice,
                                                    float* d_action_out, void* stream)
{
    LstmHPlan s;
    const int rc = build_lstm_bf16_plan(dims, n_dims, theta_and_omega_visible ? 15 : 13, s);
    if (rc != CS_OK) return rc;
    const LstmPlan& q = s.q;
    // (a length that is no whole number of floats is no blob of any network: it fails the size check as SIZE_MAX floats)
    const size_t n_floats = n_weight_bytes % sizeof(float) ? (size_t)-1 : n_weight_bytes / sizeof(float);
    // (the worlds' two arrays stand where cs_value_net_decide_lstm_bf16 has cs_lookahead's two outputs: cs_lookahead's own checks are among these)
    const int rc2 = lstm_check_decide("cs_value_net_decide_lstm_worlds_bf16", q.v, d_weights, n_floats, W, A, n, sorted_by_distance, d_next, d_current,
                                      d_actions, d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    const LstmHLds m = lstm_bf16_lds_map<LstmHLds>(s, n, 0);
    const LstmWorlds world{d_actions, d_next, d_current, d_rewards_out, m.total, theta_and_omega_visible ? 1 : 0};      // (the frame table: behind the map)
    const bool mlp1 = q.v.c0[1] > 0, wreg = q.g.ncb <= 4 * RB && s.ksh <= RKH && s.ksx <= RKX;
    const float* wb = static_cast<const float*>(d_weights);
    const int rc3 = lstm_launch(m.total + JROWS * LA_FRAME_FLOATS, W, A, wreg, mlp1, [&](auto WR, auto M1, size_t shmem, int NG, int grid) {
        constexpr auto kernel = k_value_net_lstm_worlds_bf16<decltype(WR)::value, decltype(M1)::value>;
        const int rc4 = grant_lds<kernel>(shmem);
        if (rc4 != CS_OK) return rc4;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), shmem, (hipStream_t)stream, s, m, wb, NG, A, n, sorted_by_distance, world, d_robot, robot_stride,
                           gamma, dt, d_values);
        return (int)CS_OK;
    });
    if (rc3 != CS_OK) return rc3;
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}
