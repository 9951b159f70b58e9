// lookahead.hip -- SURVEY.md §8 row f1: the robot's one-step look-ahead over its action set, batched.
// Replaces compute_rotated_states_and_reward + transform_state_to_agent_centric
//   /root/reference/crowd_nav/policy/cadrl.py:42-83, :13-39
// (called once per robot decision by CADRL / SARL / LSTM-RL: crowd_nav/policy/multi_human_rl.py:46, cadrl.py:262),
// for W robots (worlds) at once: the [W][A][n][13|15] value-network input stays on the GPU for the learner.
//
// One block per world.  Phase 1: one lane per action runs the swept collision test over the humans (sequential, with
// the reference's early break) and the agent-centric frame of that action into LDS.  Phase 2: one lane per
// (action, human) element writes a 13- or 15-float row.  The arithmetic of both phases is lookahead_math.h's, shared with the
// value-network kernels that generate the same rows in LDS (cs_value_net_decide_worlds, cs_value_net_decide_lstm_worlds[_bf16],
// cs_value_net_state).  The output is the HBM cost: 4 * 13 * A * n bytes per world (81 actions x 25 humans: 105 KB), written once;
// inputs are ~1 KB per world.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "lookahead_math.h"

namespace {

using csimpl::fail;

__global__ __launch_bounds__(256) void k_lookahead(int W, int n, int A, int headed, const float* actions, const float* next,
                                                   const float* cur, const float* robot, int rstride, float dt,
                                                   float* rotated, float* rewards)
{
    extern __shared__ float lds[]; // [A][LA_FRAME_FLOATS]: the actions' frames (LA_REWARD unused)
    const int w = blockIdx.x;
    const int nc = headed ? 6 : 4, cc = headed ? 7 : 5, oc = headed ? 15 : 13;
    const float* rb = robot + (long)w * rstride;
    const float rr = rb[4], rvd = rb[7];
    const float* curw = cur + (long)w * n * cc;
    const float* nxtw = next + (long)w * n * nc;
    for (int a = threadIdx.x; a < A; a += blockDim.x) {
        const float ax = actions[2 * a], ay = actions[2 * a + 1];
        const LaStep st = la_step(rb, ax, ay, dt);
        rewards[(long)w * A + a] = la_reward(curw, n, cc, rb, ax, ay, dt, st.dg);
        la_store_frame(lds + LA_FRAME_FLOATS * a, st, ax, ay);
    }
    __syncthreads();
    float* outw = rotated + (long)w * A * n * oc;
    for (int idx = threadIdx.x; idx < A * n; idx += blockDim.x) {
        const int a = idx / n, j = idx - a * n;
        const float* s = lds + LA_FRAME_FLOATS * a;
        const float* q = nxtw + (long)j * nc;
        const float hr = curw[(long)j * cc + 4];
        const float4 c0 = la_row_quad<0>(s, q, hr, rvd, rr, headed), c1 = la_row_quad<1>(s, q, hr, rvd, rr, headed);
        const float4 c2 = la_row_quad<2>(s, q, hr, rvd, rr, headed), c3 = la_row_quad<3>(s, q, hr, rvd, rr, headed);
        float* o = outw + (long)idx * oc;
        o[0] = c0.x; o[1] = c0.y; o[2] = c0.z; o[3] = c0.w;
        o[4] = c1.x; o[5] = c1.y; o[6] = c1.z; o[7] = c1.w;
        o[8] = c2.x; o[9] = c2.y; o[10] = c2.z; o[11] = c2.w;
        o[12] = c3.x;
        if (headed) { o[13] = c3.y; o[14] = c3.z; }
    }
}

} // namespace

extern "C" int cs_lookahead(int W, int n, int A, int theta_and_omega_visible, const float* d_actions, const float* d_next,
                            const float* d_current, const float* d_robot, int robot_stride, float dt, float* d_rotated,
                            float* d_rewards, void* stream)
{
    if (W <= 0 || n <= 0 || A <= 0) return fail(CS_ERR_ARG, "W, n, A must be positive");
    if (!d_actions || !d_next || !d_current || !d_robot || !d_rotated || !d_rewards) return fail(CS_ERR_ARG, "null argument");
    if (robot_stride < 8) return fail(CS_ERR_ARG, "robot rows need at least 8 columns: px,py,vx,vy,r,gx,gy,v_pref");
    const size_t shmem = (size_t)A * LA_FRAME_FLOATS * sizeof(float);
    if (shmem > 60 * 1024) return fail(CS_ERR_ARG, "action set too large");
    hipLaunchKernelGGL(k_lookahead, dim3(W), dim3(256), shmem, (hipStream_t)stream, W, n, A, theta_and_omega_visible ? 1 : 0,
                       d_actions, d_next, d_current, d_robot, robot_stride, dt, d_rotated, d_rewards);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}

// ---- HIP graph helpers (include/crowdstep.h) --------------------------------------------------------------
extern "C" int cs_graph_begin_capture(void* stream)
{
    if (!stream) return fail(CS_ERR_ARG, "graph capture needs a non-default stream (cs_stream_create)");
    HIP_TRY(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
    return CS_OK;
}

extern "C" int cs_graph_end_capture(void* stream, void** graph_exec)
{
    if (!stream || !graph_exec) return fail(CS_ERR_ARG, "null argument");
    hipGraph_t graph = nullptr;
    HIP_TRY(hipStreamEndCapture((hipStream_t)stream, &graph));
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return fail(CS_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    *graph_exec = exec;
    return CS_OK;
}

extern "C" int cs_graph_launch(void* graph_exec, void* stream)
{
    if (!graph_exec) return fail(CS_ERR_ARG, "null graph");
    HIP_TRY(hipGraphLaunch((hipGraphExec_t)graph_exec, (hipStream_t)stream));
    return CS_OK;
}

extern "C" int cs_graph_destroy(void* graph_exec)
{
    if (graph_exec) HIP_TRY(hipGraphExecDestroy((hipGraphExec_t)graph_exec));
    return CS_OK;
}
