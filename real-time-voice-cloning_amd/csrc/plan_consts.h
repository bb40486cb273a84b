// Launch geometry shared by the kernels (wrnn_kernels.h includes this file) and the host-only
// launch planner (plan.h / plan.cpp, built without HIP): one definition of each constant.
#pragma once

namespace wrnn {

// persistent fatchord recurrence (kernels_persist.hip)
constexpr int kPG = 8;       // groups (one per XCD)
constexpr int kPM = 32;      // workgroups per group
constexpr int kPNR = 4;      // max fold rows per group -> B <= 32
constexpr int kPH = 512;     // rnn_dims == fc_dims
// wide-row launches (kernels_persist_wide*.hip): up to kPWideRows rows per XCD group (8 kPWideRows
// per launch); the geneing 32-row ring instances (k_persist_wide_gen32) up to kPWideGen32Rows
constexpr int kPWideRows = 16;
constexpr int kPWideGen32Rows = 32;
constexpr int kMolNoise = 12;  // floats per (step, row) of the precomputed MOL noise
// persistent runtimeracer / geneing recurrences (kernels_persist_rr.hip, kernels_persist_gen.hip)
constexpr int kRH = 256;     // rnn_dims == fc_dims

}  // namespace wrnn
