// value_net_lstm_f32.h -- what the units of the float32 recurrent decision share beside value_net_lstm_kernel.h and the kernel text
// (value_net_lstm_body.inc): value_net_lstm.hip (k_value_net_lstm, k_value_net_lstm_om: rows from cs_lookahead's tensor) and
// value_net_lstm_worlds.hip (k_value_net_lstm_worlds: rows generated from the worlds).  The register-resident k-groups and the LDS map; the
// arithmetic itself is stated in value_net_lstm.hip's header comment.  Unnamed namespace: each translation unit gets its own copy.
#pragma once
#include "value_net_lstm_kernel.h"

namespace {

constexpr int RKG = 14;            // register-resident gate weights: k-groups a block (RB blocks a wavefront)
constexpr int RKG_OM = 15;         // ... of the kernel with map columns: the reference's [om] defaults are 7 blocks x (7 + 8) k-groups

struct LstmLds { int key, perm, X, XH, P, Q, J, LT, total; };

// ldg: the row stride of network 2's gather tile.  share_p: network 1's P lies over the joint rows, which are dead when mlp starts (h_n has
// gone to J, a barrier behind it) -- the kernel with map columns asks for it where P fits, to stay at two workgroups a CU with its wider rows
inline LstmLds lstm_lds_map(const LstmPlan& q, int n, int ldg = LDX, bool share_p = false)
{
    LstmLds m{};
    int o = 0;
    auto take = [&](int floats) { const int at = o; o += up(floats, 4); return at; };
    m.key = take(TILE_M * n);
    m.perm = take(TILE_M * n);
    m.XH = take(2 * TILE_M * q.ld_xh);
    m.X = q.v.c0[1] > 0 ? take(2 * TILE_M * ldg) : m.XH;
    m.P = share_p && q.v.c0[1] == 0 && q.v.ld_pq <= 2 * q.ld_xh ? m.XH : take(TILE_M * q.v.ld_pq);
    m.Q = take(TILE_M * q.v.ld_pq);
    m.J = take(JROWS * q.v.ld_j);
    m.LT = take(VN_MAX_LAYERS * 8);
    m.total = o;
    return m;
}

} // namespace
