// value_net_lstm_bf16.hip -- LSTM-RL's decision (value_net_lstm.hip: cs_value_net_decide_lstm) with the opt-in bf16 arithmetic
// (cs_value_net_decide_lstm_bf16; Python: LstmRL.set_recurrent_precision("bf16")).  The recurrent family without map columns only: networks 1
// and 2 on rows of 13 or 15 columns.  The kernel is value_net_lstm_bf16_body.inc under LSTM_OM 0; the arithmetic, its rounding points and
// the order of a chain, the tiling, the LDS images, the plan, the pack and what a decide entry does are value_net_lstm_bf16.h's, shared with
// k_value_net_lstm_om_bf16 (value_net_lstm_om_bf16.hip).  This file is the kernel's name and the two entries.
#include <hip/hip_runtime.h>

#include "value_net_lstm_bf16.h"

namespace {

template <bool WREG, bool MLP1>
__global__ __launch_bounds__(NT, 2) void k_value_net_lstm_bf16(LstmHPlan s, LstmHLds m, const float* __restrict__ wb, int NG, int A, int n, int sorted,
                                                            const float* __restrict__ rotated, const float* __restrict__ rewards,
                                                            const float* __restrict__ robot, int rstride, float gamma, float dt, float* __restrict__ values)
{
#define LSTM_OM 0
#include "value_net_lstm_bf16_body.inc"
#undef LSTM_OM
}

struct Narrow {
    static constexpr bool om = false;
    using Lds = LstmHLds;
    template <bool WREG, bool MLP1> static constexpr auto kernel = k_value_net_lstm_bf16<WREG, MLP1>;
};

} // namespace

#include "value_net_pick.h"

extern "C" int cs_value_net_pack_lstm_bf16(const int32_t* dims, int n_dims, int cols, const float* const* params, void* blob, size_t* n_bytes)
{
    LstmHPlan s;
    const int rc = build_lstm_bf16_plan(dims, n_dims, cols, s);
    if (rc != CS_OK) return rc;
    return pack_lstm_bf16_blob(s, 0, params, blob, n_bytes);
}

extern "C" int cs_value_net_decide_lstm_bf16(const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n, int cols,
                                             int sorted_by_distance, const float* d_rotated, const float* d_rewards, const float* d_actions,
                                             const float* d_robot, int robot_stride, float gamma, float dt, const int32_t* d_override, float* d_values,
                                             int32_t* d_choice, float* d_action_out, void* stream)
{
    return lstm_bf16_decide<Narrow>("cs_value_net_decide_lstm_bf16", dims, n_dims, d_weights, n_weight_bytes, W, A, n, cols, 0, sorted_by_distance,
                                    CS_VN_MAPS_OWN, d_rotated, nullptr, d_rewards, d_actions, d_robot, robot_stride, gamma, dt, d_override, d_values,
                                    d_choice, d_action_out, stream);
}
