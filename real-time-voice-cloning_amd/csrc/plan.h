// The launch planner of the persistent engine: the rate table,
// the per-call launch plan and the streams a planned call writes. Plain C++ (plan.cpp, no HIP):
// runtime.hip fills a PlanIn from the handle and the device (plan_inputs) and runs what comes back.
#pragma once
#include <string>
#include <vector>

#include "plan_consts.h"

namespace wrnn {

// ===== Launch-plan rates ==================================================
// Per-step costs (us, MI355X) the launch planner minimises. The defaults are the measured
// points of the rounds cited beside them; a measurement pass emits a per-build table
// (tools/make_rates.py -> wavernn_amd/rates_mi355x.txt next to the library, or the file named
// by env WRNN_RATES) that replaces them key by key at wrnn_create. Format: one key per line,
// `name v1 v2 ...`, '#' comments; by rows per group 1..4 for the register-resident tables.
struct PlanRates {
    double fat9[kPNR + 1] = {0, 4.8, 5.15, 5.91, 6.92};   // k_persist 9-bit (r05 nr_probe)
    double fat10[kPNR + 1] = {0, 4.21, 5.19, 6.50, 9.41}; // 10-bit (profiles/r06/b u10_nr*)
    // sparse instances (§3.0g): 9-bit measured (profiles/r06/b sp_nr*, 90 %-pruned weights);
    // 10-bit = 9-bit + the dense 10-bit / 9-bit difference at 3-4 rows (estimate)
    double fat9_sp[kPNR + 1] = {0, 4.99, 6.95, 7.99, 9.26};
    double fat10_sp[kPNR + 1] = {0, 5.3, 7.3, 8.6, 11.7};
    double rr[kPNR + 1] = {0, 6.7, 7.75, 8.81, 9.87};     // k_persist_rr (round 2, linear below 3)
    double gen[kPNR + 1] = {0, 2.61, 3.26, 3.91, 4.56};   // k_persist_gen
    // wide MFMA launches: base + row x r per step at r rows per group, + c10 at 1024 classes:
    // 9.72 us at 16 rows (profiles/r05/final/c4.log, r06/b sp_c4), 10.965 at 16 rows / 1024
    // classes (r05/final/b10.log), 10.59 at 6 rows / 1024 classes (r06/b u10_wide)
    double wide[3] = {9.32, 0.025, 1.24};
    // block-sparse wide launches of a pruned fatchord RAW model (k_persist_wide_sp, §3.0g the wide
    // form; offered only where the sparse-wide image exists), same three terms: 23.03 / 23.47 / 24.32
    // us at 5 / 9 / 16 rows per group on 90 %-pruned weights, 24.40 / 24.97 / 26.00 at 1024 classes
    // (profiles/wide_sp/rates.log; the least-squares form of tools/make_rates.py) -- slower than
    // the dense wide kernel (9.55 / 9.69 / 9.76), so by rate every launch stays dense
    double wide_sp[3] = {22.434, 0.1173, 1.518};
    // the MOL head on the wide kernel (fatchord): base + row x r. 9.43 / 9.57 / 9.65 us at 5 / 9 /
    // 16 rows per group (profiles/wide_mol/mol_wide_r*.log, least squares: tools/make_rates.py)
    double wide_mol[2] = {9.366, 0.0185};
    double wide_rr[2] = {12.0, 0.025};                     // 12.39 us at 15-16 rows (r04 wide_rr)
    // the MOL head on the runtimeracer wide kernel: base + row x r. 9.43 / 9.60 / 9.79 us at 5 / 9 /
    // 16 rows per group (profiles/wide_rr_mol/rr_mol_wide_r*.log, least squares:
    // tools/make_rates.py)
    double wide_rr_mol[2] = {9.285, 0.0321};
    // geneing BITS on its wide kernel (kernels_persist_wide_gen.hip): base + row x r. 3.540 /
    // 3.594 / 3.634 us at 5 / 9 / 16 rows per group (profiles/wide_gen/gen_wide_r*.log, least
    // squares: tools/make_rates.py)
    double wide_gen[2] = {3.508, 0.0082};
    // the geneing continuous heads on the same kernel, base + row x r: MOL (30 logits) 3.067 /
    // 3.116 / 3.172 us, Beta (2 logits, float64 gamma draws) 4.993 / 5.156 / 5.361 us at 5 / 9 / 16
    // rows per group (profiles/wide_gen_mol/gen_{mol,beta}_wide_r*.log, least squares:
    // tools/make_rates.py)
    double wide_gen_mol[2] = {3.025, 0.0094};
    double wide_gen_beta[2] = {4.84, 0.033};
    // the 32-row ring instances of that kernel (k_persist_wide_gen32; launches of 17 .. 32 rows per
    // group, wrnn_set_gen_wide_rows(32)), base + row x r: BITS 6.476 / 6.464 / 6.555 us, MOL 4.411 /
    // 4.422 / 4.677 us, Beta 7.413 / 7.932 / 8.415 us at 17 / 23 / 29 rows per group
    // (profiles/wide_gen32/gen32_{,mol_,beta_}wide_r*.log, least squares: tools/make_rates.py)
    double wide_gen32[2] = {6.347, 0.0066};
    double wide_gen32_mol[2] = {3.992, 0.0222};
    double wide_gen32_beta[2] = {6.001, 0.0835};
    // the time-sliced instances of that kernel (k_persist_wide_gen_rot, wrnn_set_gen_wide_slices),
    // base + row x r: BITS 3.591, MOL 2.947, Beta 5.256 us per step at 16 rows per group, the medians
    // of nine sliced calls each (profiles/wide_gen_slices/gen_slice{,_mol,_beta}_r16.log); a sliced
    // launch runs 16 rows per group but for the short tails, so the per-row terms are the unsliced
    // keys' (tools/make_rates.py)
    double wide_gen_slice[2] = {3.46, 0.0082};
    double wide_gen_slice_mol[2] = {2.797, 0.0094};
    double wide_gen_slice_beta[2] = {4.728, 0.033};
    double slice[2] = {60.0, 0.98};                        // us per extra launch, gain threshold
    // rotation: rates of the rotated instance's two bodies by rows per group (the (q + 1)-row
    // one at its single-launch rate; the q-row one the best split measured, §3.0e)
    double rot9[kPNR + 1] = {0, 4.8, 5.22, 5.91, 6.92};
    double rot9_sp[kPNR + 1] = {0, 4.99, 6.95, 7.99, 9.26};  // sparse (r06/b sp_nr*)
    double rot_mol3_lo = 4.70;                             // MOL 3-row split (r05 rotation scan)
    double rot_rr9[kPNR + 1] = {0, 6.3, 7.0, 7.78, 8.8};   // (2 / 4 rows: estimates)
    double rot_rr10[kPNR + 1] = {0, 6.5, 7.26, 8.14, 9.23};  // profiles/r05/rr_rates/
    double rot_rrm[kPNR + 1] = {0, 5.9, 6.6, 7.42, 8.4};   // profiles/r05/rr_rotation/mol/
    double rot_gen[kPNR + 1] = {0, 1.98, 2.47, 3.12, 3.64};  // profiles/r05/gen_rotation/
    double rot_genm[kPNR + 1] = {0, 1.72, 2.15, 2.60, 3.03};
    double rot[2] = {40.0, 0.98};                          // us per extra launch, gain threshold
    std::string source = "built-in defaults";
};

// Overrides the keys a table names (unknown keys and malformed lines are errors; values must
// be positive). The register-resident tables take 1-4 values (rows per group 1..4).
bool parse_rates(const char* text, PlanRates& R, std::string& err);
std::string rates_text(const PlanRates& R);
// The table a new handle plans with: the defaults, then WRNN_RATES (a path) or the
// rates_mi355x.txt beside this library when present. A file that does not parse is reported on
// stderr and ignored (the defaults stay).
PlanRates load_rates();

// ===== Launches ==============================================================================
struct PLaunch {
    int rb, nr;  // first row, rows per XCD group (the launch runs rows rb + g + 8 r, r < nr)
    bool wide;   // kernels_persist_wide.hip (MFMA) or the register-resident kernel
    int rot = -1;  // launch j of the call's row rotation (rot_plan), or -1
    bool sp = false;  // a wide launch priced (and to be run) as block-sparse wide (rate key wide_sp)
};
// One entry of a virtual-row map: virtual row g + 8 r of a rotated or time-sliced launch runs
// physical row `row` from step `off` (the kernels read the uploaded maps as int2)
struct VRow {
    int row, off;
};
// Row rotation of a call: per launch j the virtual-row map, rows and steps per
// group, and the launch's RowInfo table
struct RotPlan {
    int K = 0, nr_hi = 0, n_hi = 0, n_lo = 0;
    std::vector<VRow> vmap;     // [K][kPG * nr_hi]
    std::vector<int> gnr, git;  // [K][kPG]
};
// Time-sliced wide launches of a call: per launch the rows per group, the steps
// and the virtual-row map, by virtual row g + 8 r
struct WLaunch {
    int nr, steps;
    std::vector<VRow> vmap;  // [kPG * nr]
};

bool plan_rotation(int R, int S, double t_hi, double t_lo, RotPlan& P, double launch_us = 40.0,
                   double gain = 0.98);
bool plan_wide_slices(int R, int S, std::vector<WLaunch>& out);

// Inputs of one call's launch plan: the model, the call's rows / steps, which kernel variants
// exist and spill (scratch bytes, -1 = no such variant) and the env switches. generate_impl
// fills it from the handle and the device; wrnn_debug_plan from its arguments (spill-free).
struct PlanIn {
    bool ok = false, fat = false, rr = false, gen = false;
    int mode = 0, n = 0, cpw = 0, B = 0, S = 0;
    bool c10 = false, sp = false, p1ring = false, rr_frames = false;
    bool force_sp = false;  // env WRNN_SPARSE=1: the sparse instances whatever the rates
    bool has_wide = false;  // the wide image of this call's head (topology and mode) exists
    // fatchord RAW: the block-sparse wide image exists too (sparse_wide_pack.h: the pruned weights'
    // lists fit); sp_wide_mode: env WRNN_SPARSE_WIDE, 0 never, 1 every wide launch, -1 by rate
    bool has_wide_sp = false;
    int sp_wide_mode = -1;
    // geneing: the head's 32-row ring instances are selected (wrnn_set_gen_wide_rows / env
    // WRNN_GEN_WIDE_ROWS) and can run -- spill-free, and the call can take the ring (the per-frame
    // P1 form exists, WRNN_GEN_RING is not 0): established before a 32-row launch is priced
    bool gen32 = false;
    // geneing: the head's time-sliced ring instances are selected (wrnn_set_gen_wide_slices / env
    // WRNN_GEN_SLICE) and can run, under the same conditions
    bool gen_slices = false;
    int scr[2][kPNR + 1] = {};     // fatchord k_persist [stream | ring][nr]
    int scr_sp[kPNR + 1] = {};     // sparse instances
    int scr_rot[2][kPNR + 1] = {}; // rotated instance of this topology / mode [dense | sparse][nr]
    bool ok_reg[kPNR + 1] = {};    // runtimeracer / geneing register-resident variants
    int wide_scr = 0, wide_rot_scr = 0;
    // env switches
    int wmode = 2, nr_max = 0;
    bool slice_off = false, rot_off = false, allow_wide_scratch = false;
    double rot_hi = 0, rot_lo = 0;  // WRNN_ROT_US (rate A/B); 0: none
};
struct PlanOut {
    std::vector<PLaunch> lplan;
    double plan_us = 0;
    std::vector<WLaunch> wrot;
    RotPlan rot;
    bool p1_ring = false, sparse = false;
    int Bplan = 0;
};
void plan_call(const PlanIn& in, const PlanRates& R, PlanOut& out);

constexpr double kPersistWsBytes = 96.0 * (1 << 30);  // P1 + cI + noise cap (of 288 GB HBM)
struct StreamPlan {
    double p1_bytes = 0, noise_bytes = 0;
    bool p1_stream = true, gen_ring = false, persist_ok = false;
};
StreamPlan plan_streams(const PlanIn& in, const PlanOut& out, bool p1x4, bool gen_frames, int sw);

constexpr int kPlanRowsMax = 1 << 20;  // wrnn_debug_plan: far above any call (C4 is 144 rows per GPU)
// PlanIn of a described call (wrnn_debug_plan, wrnn_debug_stream_bytes): every variant spill-free.
// Returns WRNN_OK or the error it reported.
int debug_plan_in(int model_type, int bits, int mode, int rows, int seq_len, int flags, PlanIn& in);

}  // namespace wrnn
