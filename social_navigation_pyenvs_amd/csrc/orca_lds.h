// orca_lds.h -- the dynamic LDS of the four ORCA kernels (orca.hip), described ONCE: the kernel takes its pointers from the regions'
// offsets, the host takes the launch's byte count from `total`.  Plain C++ (tests/test_orca_lds_cpu.py compiles it with g++).
// A region is [count] elements of 16 (float4), 8 (float2) or 4 (float, int) bytes; regions follow one another without padding, in an
// order that keeps each aligned for its element (the float2 chords come 72 at a time: 576 bytes, a multiple of 16).
#pragma once

#ifdef __HIPCC__
#define ORCA_LDS_FN __host__ __device__ inline
#else
#define ORCA_LDS_FN inline
#endif

namespace csimpl {

struct LdsSpan { unsigned off, bytes; };
struct LdsCarver {
    unsigned at;
    ORCA_LDS_FN LdsSpan take(int count, unsigned elem) { const LdsSpan s{at, (unsigned)count * elem}; at += s.bytes; return s; }
};
constexpr int LP3_ROWS_SLOTS = 72;   // lp3_rows: [9][8] projected lines (float4) and their chords (float2) of the eight rows in flight

// k_orca_step<FAST10, MAXT, FM>: T lanes, wpb worlds of `rows` rows each; the per-lane columns are TL = wpb * rows lanes wide.
// The register-resident build (fast10) keeps a copy of its ten lines for linearProgram3 and, unless lp3_static, lp3_rows' regions;
// the generic build keeps K + KO lines, as many projected lines, K neighbours and KO obstacle edges per lane.
struct OrcaStepLds { LdsSpan pv, L, P, rowP, rowA, q, r, nd, ni, rp, g0x, flag, od, oi, sel; unsigned total; };
ORCA_LDS_FN OrcaStepLds orca_step_lds(bool fast10, bool lp3_static, int T, int wpb, int rows, int K, int KO)
{
    const int TL = wpb * rows, KL = fast10 ? 0 : K + KO, KN = fast10 ? 0 : K, RS = (fast10 && !lp3_static) ? LP3_ROWS_SLOTS : 0, TF = fast10 ? T : 0;
    LdsCarver c{0};
    OrcaStepLds o;
    o.pv = c.take(2 * T, 16);                    // [2][T] x, y, vx, vy
    o.L = c.take((fast10 ? 10 : KL) * TL, 16);   // [KL][TL] ORCA lines
    o.P = c.take(KL * TL, 16);                   // [KL][TL] LP3 projection lines
    o.rowP = c.take(RS, 16);                     // lp3_rows: projected lines,
    o.rowA = c.take(RS, 8);                      // their chords,
    o.q = c.take(TF, 16);                        // [T] (result, maxSpeed, distance) per agent
    o.r = c.take(T, 4);                          // [T] radius + margin
    o.nd = c.take(KN * TL, 4);                   // [K][TL] neighbour distSq
    o.ni = c.take(KN * TL, 4);                   // [K][TL] neighbour row
    o.rp = c.take(T, 4);                         // [T] plain radius (respawn rule)
    o.g0x = c.take(T, 4);                        // [T] respawn scratch
    o.flag = c.take(T, 4);                       // [T] respawn scratch
    o.od = c.take(KO * TL, 4);                   // [KO][TL] obstacle edge distSq
    o.oi = c.take(KO * TL, 4);                   // [KO][TL] obstacle edge (first vertex)
    o.sel = c.take(TF, 4);                       // [T] lp3_rows tickets
    o.total = c.at;
    return o;
}

// k_orca_robot_step: one lane per world, columns 64 lanes wide
struct OrcaRobotLds { LdsSpan L, P, nd, ni, od, oi; unsigned total; };
ORCA_LDS_FN OrcaRobotLds orca_robot_lds(int K, int KO)
{
    LdsCarver c{0};
    OrcaRobotLds o;
    o.L = c.take((K + KO) * 64, 16);             // [K + KO][64] ORCA lines
    o.P = c.take((K + KO) * 64, 16);             // [K + KO][64] LP3 projection lines
    o.nd = c.take(K * 64, 4);                    // [K][64] neighbour distSq
    o.ni = c.take(K * 64, 4);                    // [K][64] neighbour row
    o.od = c.take(KO * 64, 4);                   // [KO][64] obstacle edge distSq
    o.oi = c.take(KO * 64, 4);                   // [KO][64] obstacle edge
    o.total = c.at;
    return o;
}

// k_orca_robot_step_fast: wpb worlds per block, n humans and the robot itself as the last row of each
struct OrcaRobotFastLds { LdsSpan pv, rr, ln, pr, pa, q, sel; unsigned total; };
ORCA_LDS_FN OrcaRobotFastLds orca_robot_fast_lds(int wpb, int n)
{
    const int ent = wpb * (n + 1);
    LdsCarver c{0};
    OrcaRobotFastLds o;
    o.pv = c.take(ent, 16);                      // [wpb][n + 1] x, y, vx, vy
    o.rr = c.take((ent + 3) & ~3, 4);            // [wpb][n + 1] radius + margin (padded to the next float4)
    o.ln = c.take(10 * 64, 16);                  // [10][64] the lanes' ORCA lines for LP3
    o.pr = c.take(LP3_ROWS_SLOTS, 16);           // lp3_rows: projected lines,
    o.pa = c.take(LP3_ROWS_SLOTS, 8);            // their chords,
    o.q = c.take(64, 16);                        // [64] agent records
    o.sel = c.take(64, 4);                       // [64] tickets
    o.total = c.at;
    return o;
}

// k_bw_orca_step<FAST10>: 64 agents per block.  The register-resident build has lp3_rows' regions whatever lp3_static says.
struct OrcaGridLds { LdsSpan ln, pr, pa, q, sel, nd, ni, od, oi; unsigned total; };
ORCA_LDS_FN OrcaGridLds orca_grid_lds(bool fast10, int K, int KO)
{
    const int KL = fast10 ? 10 : K + KO, KN = fast10 ? 0 : K, KOB = fast10 ? 0 : KO, RS = fast10 ? LP3_ROWS_SLOTS : 0, TF = fast10 ? 64 : 0;
    LdsCarver c{0};
    OrcaGridLds o;
    o.ln = c.take(KL * 64, 16);                  // [KL][64] ORCA lines
    o.pr = c.take(fast10 ? RS : KL * 64, 16);    // fast10: lp3_rows projections; generic: [KL][64] LP3 projection lines
    o.pa = c.take(RS, 8);                        // fast10: their chords
    o.q = c.take(TF, 16);                        // fast10: [64] agent records
    o.sel = c.take(TF, 4);                       // fast10: [64] tickets
    o.nd = c.take(KN * 64, 4);                   // generic: [K][64] neighbour distSq
    o.ni = c.take(KN * 64, 4);                   // generic: [K][64] neighbour row
    o.od = c.take(KOB * 64, 4);                  // generic: [KO][64] obstacle edge distSq
    o.oi = c.take(KOB * 64, 4);                  // generic: [KO][64] obstacle edge
    o.total = c.at;
    return o;
}

} // namespace csimpl
