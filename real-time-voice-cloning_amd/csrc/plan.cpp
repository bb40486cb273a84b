// The launch planner (plan.h): rate table, per-call launch plan, stream plan, and the handle-free
// wrnn_debug_* entry points that expose them to the CPU tests. No HIP: built by g++ like binfile.cpp.
#include "plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include <dlfcn.h>

#include "wavernn_mi355x.h"

extern "C" int wrnn_internal_fail(int code, const char* msg);  // runtime.hip

namespace wrnn {

namespace {

int fail(int code, const std::string& msg) { return wrnn_internal_fail(code, msg.c_str()); }

// One row per key of the table format: its name, the first value of its storage and the value
// count (the register-resident tables keep their unused slot 0: values for 1..4 rows per group).
using RateAt = const double* (*)(const PlanRates&);
#define RATE_AT(expr) [](const PlanRates& R) -> const double* { return expr; }
struct RateKey {
    const char* name;
    RateAt at;
    int n;
};
const RateKey kRateKeys[] = {
    {"fat9", RATE_AT(R.fat9 + 1), kPNR},
    {"fat10", RATE_AT(R.fat10 + 1), kPNR},
    {"fat9_sp", RATE_AT(R.fat9_sp + 1), kPNR},
    {"fat10_sp", RATE_AT(R.fat10_sp + 1), kPNR},
    {"rr", RATE_AT(R.rr + 1), kPNR},
    {"gen", RATE_AT(R.gen + 1), kPNR},
    {"wide", RATE_AT(R.wide), 3},
    {"wide_sp", RATE_AT(R.wide_sp), 3},
    {"wide_mol", RATE_AT(R.wide_mol), 2},
    {"wide_rr", RATE_AT(R.wide_rr), 2},
    {"wide_rr_mol", RATE_AT(R.wide_rr_mol), 2},
    {"wide_gen", RATE_AT(R.wide_gen), 2},
    {"wide_gen_mol", RATE_AT(R.wide_gen_mol), 2},
    {"wide_gen_beta", RATE_AT(R.wide_gen_beta), 2},
    {"wide_gen32", RATE_AT(R.wide_gen32), 2},
    {"wide_gen32_mol", RATE_AT(R.wide_gen32_mol), 2},
    {"wide_gen32_beta", RATE_AT(R.wide_gen32_beta), 2},
    {"wide_gen_slice", RATE_AT(R.wide_gen_slice), 2},
    {"wide_gen_slice_mol", RATE_AT(R.wide_gen_slice_mol), 2},
    {"wide_gen_slice_beta", RATE_AT(R.wide_gen_slice_beta), 2},
    {"slice", RATE_AT(R.slice), 2},
    {"rot9", RATE_AT(R.rot9 + 1), kPNR},
    {"rot9_sp", RATE_AT(R.rot9_sp + 1), kPNR},
    {"rot_mol3_lo", RATE_AT(&R.rot_mol3_lo), 1},
    {"rot_rr9", RATE_AT(R.rot_rr9 + 1), kPNR},
    {"rot_rr10", RATE_AT(R.rot_rr10 + 1), kPNR},
    {"rot_rrm", RATE_AT(R.rot_rrm + 1), kPNR},
    {"rot_gen", RATE_AT(R.rot_gen + 1), kPNR},
    {"rot_genm", RATE_AT(R.rot_genm + 1), kPNR},
    {"rot", RATE_AT(R.rot), 2},
};

// The wide MFMA head of a (topology, mode): what plan_call needs to price and admit its launches.
// An empty entry (no key): the head has no wide kernel (wrnn_create refuses Beta for fatchord and
// runtimeracer, so no handle reaches those).
struct WideHead {
    RateAt key;       // per step at r rows per group: key[0] + key[1] r ...
    bool c10_term;    // ... + key[2] at 1024 classes
    bool above_reg;   // offered only to calls no single register-resident launch holds (more than
                      // kPG * kPNR rows: smaller plans stay as they were) or with WRNN_PERSIST_WIDE=1
    bool mol_bound;   // its launches index the k_mol_noise stream in 32 bits (wide_fits below)
    int max_scratch;  // scratch bytes accepted (Beta: the frame k_persist_gen BETA is accepted with)
    RateAt key32;     // geneing: the 32-row ring instances' key (17 .. 32 rows per group)
    bool slices;      // time-sliced launches are planned by default (P1 formed in-kernel: fatchord ring,
                      // runtimeracer); geneing has them opt-in (PlanIn::gen_slices) ...
    RateAt key_slice; // ... on instances of their own, priced by their own key
};
const WideHead kWideHeads[3][3] = {  // [fatchord | runtimeracer | geneing][RAW | MOL | Beta]
    {{RATE_AT(R.wide), true, false, false, 0, nullptr, true},
     {RATE_AT(R.wide_mol), false, false, true, 0, nullptr, true}},
    {{RATE_AT(R.wide_rr), false, false, false, 0, nullptr, true},
     {RATE_AT(R.wide_rr_mol), false, true, true, 0, nullptr, true}},
    // (the geneing kernel forms the MOL stream's address of every step in 64 bits: its 16-row
    // launches have no 2-GiB bound; plan_call holds only the 32-row plan to one)
    {{RATE_AT(R.wide_gen), false, true, false, 0, RATE_AT(R.wide_gen32), false, RATE_AT(R.wide_gen_slice)},
     {RATE_AT(R.wide_gen_mol), false, true, false, 0, RATE_AT(R.wide_gen32_mol), false, RATE_AT(R.wide_gen_slice_mol)},
     {RATE_AT(R.wide_gen_beta), false, true, false, 16, RATE_AT(R.wide_gen32_beta), false,
      RATE_AT(R.wide_gen_slice_beta)}},
};

int gcd_i(int a, int b) { return b ? gcd_i(b, a % b) : a; }

}  // namespace

bool parse_rates(const char* text, PlanRates& R, std::string& err) {
    std::istringstream in(text ? text : "");
    std::string line;
    int ln = 0;
    while (std::getline(in, line)) {
        ++ln;
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.resize(hash);
        std::istringstream ls(line);
        std::string key;
        if (!(ls >> key)) continue;
        std::vector<double> v;
        double x;
        while (ls >> x) v.push_back(x);
        if (!ls.eof()) return err = "line " + std::to_string(ln) + ": not a number", false;
        const RateKey* k = nullptr;
        for (const auto& e : kRateKeys)
            if (key == e.name) k = &e;
        if (!k) return err = "line " + std::to_string(ln) + ": unknown key '" + key + "'", false;
        for (double d : v)
            if (!(d > 0)) return err = "line " + std::to_string(ln) + ": values must be > 0", false;
        if (v.size() != (size_t)k->n)
            return err = "line " + std::to_string(ln) + ": '" + key + "' takes " + std::to_string(k->n) + " values",
                   false;
        std::copy(v.begin(), v.end(), const_cast<double*>(k->at(R)));  // (R itself is not const)
    }
    return true;
}

std::string rates_text(const PlanRates& R) {
    std::ostringstream o;
    o << "# source: " << R.source << "\n";
    for (const auto& k : kRateKeys) {
        o << k.name;
        for (int i = 0; i < k.n; ++i) o << ' ' << k.at(R)[i];
        o << '\n';
    }
    return o.str();
}

PlanRates load_rates() {
    PlanRates R;
    std::string path;
    if (const char* e = std::getenv("WRNN_RATES")) {
        path = e;
    } else {
        Dl_info di;
        if (dladdr(reinterpret_cast<void*>(&load_rates), &di) && di.dli_fname) {
            std::string so = di.dli_fname;
            const size_t sl = so.rfind('/');
            path = (sl == std::string::npos ? std::string(".") : so.substr(0, sl)) + "/rates_mi355x.txt";
        }
    }
    if (path.empty()) return R;
    std::ifstream f(path);
    if (!f) return R;
    std::stringstream ss;
    ss << f.rdbuf();
    PlanRates T = R;
    std::string err;
    if (!parse_rates(ss.str().c_str(), T, err)) {
        std::fprintf(stderr, "[wavernn-mi355x] WARNING: rate table %s ignored: %s\n", path.c_str(), err.c_str());
        return R;
    }
    T.source = path;
    return T;
}

// Row rotation. R fold rows on the 8 XCD groups of one register-resident
// launch leave m = R % 8 groups with q + 1 rows and 8 - m with q: every group pays the
// (q + 1)-row step (a padding row costs as much as a real one), so the launch runs S steps at
// t(q + 1). Rotating the rows through the q + 1-row groups over K launches -- each row spends
// h_c of them in a q + 1-row group and l_c in a q-row group, a group of q rows running its own
// q-row body (the rotated kernel instance holds both) -- lets every group run at its own rate:
// a q + 1-row group runs n_hi steps, a q-row group n_lo, n_hi t(q + 1) ~ n_lo t(q), and
// h_c n_hi + l_c n_lo = S for every row. A row's state crosses launches through the chunk state
// (st_*); its noise, labels and frames are read at its own step (the map's offset).
// C2 (18 rows): 3 launches, 3672 steps at 3 rows / 4214 at 2 -> 65.1 ms instead of 71.5.
bool plan_rotation(int R, int S, double t_hi, double t_lo, RotPlan& P, double launch_us, double gain) {
    P = RotPlan();
    const int q = R / kPG, m = R % kPG;
    if (q < 1 || m == 0 || q + 1 > 3 || S < 64) return false;
    const int H = m * (q + 1), gg = gcd_i(R, H), K = R / gg, hc = H / gg, lc = K - hc;
    if (K > 24 || lc < 1) return false;
    // n_hi t_hi = n_lo t_lo and hc n_hi + lc n_lo = S, in integers
    const double nh0 = S / (hc + lc * t_hi / t_lo);
    int nh = -1, nl = -1;
    for (int d = 0; d <= lc && nh < 0; ++d)
        for (int sgn = -1; sgn <= 1 && nh < 0; sgn += 2) {
            const int c = (int)std::lround(nh0) + sgn * d;
            if (c >= 1 && (S - hc * c) > 0 && (S - hc * c) % lc == 0) {
                nh = c;
                nl = (S - hc * c) / lc;
            }
        }
    if (nh < 1 || nl < 1) return false;
    // worth it? (an extra launch reloads the weights: ~40 us)
    const double rot = K * std::max(nh * t_hi, nl * t_lo) + (K - 1) * launch_us, plain = S * t_hi;
    if (rot > gain * plain) return false;
    P.K = K;
    P.nr_hi = q + 1;
    P.n_hi = nh;
    P.n_lo = nl;
    P.vmap.assign((size_t)K * kPG * (q + 1), VRow{0, 0});
    P.gnr.assign((size_t)K * kPG, 0);
    P.git.assign((size_t)K * kPG, 0);
    std::vector<int> off(R, 0);
    for (int j = 0; j < K; ++j) {
        std::vector<char> hi(R, 0);
        std::vector<int> his, los;
        for (int i = 0; i < H; ++i) hi[(j * gg + i) % R] = 1;
        for (int i = 0; i < H; ++i) his.push_back((j * gg + i) % R);
        for (int r = 0; r < R; ++r)
            if (!hi[r]) los.push_back(r);
        for (int g = 0; g < kPG; ++g) {
            const bool gh = g < m;
            const int nr = gh ? q + 1 : q;
            P.gnr[(size_t)j * kPG + g] = nr;
            P.git[(size_t)j * kPG + g] = gh ? nh : nl;
            for (int r = 0; r < nr; ++r) {
                const int row = gh ? his[(size_t)g * (q + 1) + r] : los[(size_t)(g - m) * q + r];
                P.vmap[(size_t)j * kPG * (q + 1) + g + kPG * r] = VRow{row, off[row]};
            }
        }
        for (int r = 0; r < R; ++r) off[r] += hi[r] ? nh : nl;
    }
    for (int r = 0; r < R; ++r)
        if (off[r] != S) return (P = RotPlan(), false);
    return true;
}

// Time-sliced wide launches. The wide kernel's step costs nearly the same for
// any row count up to 16 per group (MFMA tiles of 16 columns), so R = 8 R_g rows with R_g > 16
// (not a multiple of 16; at most 64 launches) run best as launches of 16 rows per group over
// rotating row sets: with
// d = R_g - 16 rows of each group idle per launch (a circular shift by gcd(R_g, d) rows per
// launch), K = R_g / gcd launches make every row active in A = 16 K / R_g of them; each runs
// n = S / A steps (integer part), and ceil(R_g / 16) short launches give every row the remaining
// S - A n. C4 (144 rows, 18 per group): 9 launches of 1,512 steps + 2 of 4 -- 1.125 S wide steps
// instead of S wide steps + S steps of a 2-row register-resident launch for the 16 rows left over.
bool plan_wide_slices(int R, int S, std::vector<WLaunch>& out) {
    out.clear();
    if (R % kPG) return false;
    const int Rg = R / kPG;
    if (Rg <= kPWideRows || Rg % kPWideRows == 0) return false;  // (a multiple of 16: full launches)
    const int d = Rg - kPWideRows, gg = gcd_i(Rg, d), K = Rg / gg, A = kPWideRows * K / Rg;
    if (K > 64) return false;
    const int n = S / A, rem = S - A * n;
    if (n < 64) return false;
    std::vector<int> off(R, 0);
    for (int j = 0; j < K; ++j) {
        std::vector<char> idle(Rg, 0);
        for (int k = 0; k < d; ++k) idle[(j * gg + k) % Rg] = 1;
        WLaunch L{kPWideRows, n, std::vector<VRow>((size_t)kPG * kPWideRows)};
        for (int g = 0; g < kPG; ++g) {
            int r = 0;
            for (int i = 0; i < Rg; ++i)
                if (!idle[i]) {
                    const int row = g + kPG * i;
                    L.vmap[(size_t)g + kPG * r++] = VRow{row, off[row]};
                    off[row] += n;
                }
        }
        out.push_back(std::move(L));
    }
    for (int k = 0; rem > 0 && k * kPWideRows < Rg; ++k) {  // the remaining steps of every row
        const int nr = std::min(kPWideRows, Rg - k * kPWideRows);
        WLaunch L{nr, rem, std::vector<VRow>((size_t)kPG * nr)};
        for (int g = 0; g < kPG; ++g)
            for (int r = 0; r < nr; ++r) {
                const int row = g + kPG * (k * kPWideRows + r);
                L.vmap[(size_t)g + kPG * r] = VRow{row, off[row]};
                off[row] += rem;
            }
        out.push_back(std::move(L));
    }
    for (int r = 0; r < R; ++r)
        if (off[r] != S) return (out.clear(), false);
    return true;
}

// The persistent launch plan (consecutive launches over row batches; launch k runs rows
// rb_k + g + 8 r, r < nr_k, in every XCD group g): the cheapest mix of register-resident
// (nr <= 4, spill-free variants) and wide MFMA launches (nr <= 16; geneing with 32 rows selected:
// nr <= 32 in plans of wide launches only) by the per-step rates, then
// time-sliced wide launches (§3.0f) or a row rotation (§3.0e) when those are cheaper.
void plan_call(const PlanIn& in, const PlanRates& R, PlanOut& out) {
    out = PlanOut();
    const int B = in.B, S = in.S;
    const bool mol = in.mode == WRNN_MODE_MOL;
    // the wide head of this call, when its image exists
    const WideHead* hd = nullptr;
    if (in.ok && in.has_wide && in.mode >= 0 && in.mode <= 2) hd = &kWideHeads[in.fat ? 0 : in.rr ? 1 : 2][in.mode];
    if (hd && !hd->key) hd = nullptr;
    // per-step cost of one of its launches of r rows per group
    auto wide_us = [&](int r) {
        const double* k = hd->key(R);
        return k[0] + k[1] * r + (hd->c10_term && in.c10 ? k[2] : 0.0);
    };
    // fatchord RAW with the block-sparse wide image: a wide launch of r rows per group runs sparse
    // when forced or when its key is strictly cheaper, and is priced with the one it runs
    const bool sp_head = hd && in.fat && in.mode == WRNN_MODE_RAW && in.has_wide_sp && in.sp_wide_mode != 0;
    auto wide_sp_us = [&](int r) { return R.wide_sp[0] + R.wide_sp[1] * r + (in.c10 ? R.wide_sp[2] : 0.0); };
    auto wide_is_sp = [&](int r) { return sp_head && (in.sp_wide_mode == 1 || wide_sp_us(r) < wide_us(r)); };
    auto wide_cost = [&](int r) { return wide_is_sp(r) ? wide_sp_us(r) : wide_us(r); };
    // a wide MOL launch indexes the k_mol_noise stream ([S][rows][kMolNoise], rows padded to a
    // launch) in 32 bits: it must stay below 2 GiB (launch_persist_wide and
    // launch_persist_wide_rr refuse it otherwise)
    const bool wide_fits = !mol || (double)S * (B + kPG * kPWideRows) * kMolNoise * 4.0 < 2147483648.0;
    // ... and the call is one the head takes (its scratch and WRNN_PERSIST_WIDE=0 aside)
    const bool head_ok = hd && (!hd->mol_bound || wide_fits) &&
                         (!hd->above_reg || in.wmode == 1 || B > kPG * kPNR);
    struct Opt {
        int nr;
        bool wide;
        double us;
    };
    // sparse k_persist instances compete with the dense ones by their own rates: the cheaper
    // register-resident family wins the call (both give the same results, §3.0g)
    const double* us = in.c10 ? R.fat10 : R.fat9;
    const double* us_sp = in.c10 ? R.fat10_sp : R.fat9_sp;
    // a fatchord register-resident variant runs with at most 64 bytes of scratch; with the P1 ring
    // the call uses the flavour (stream | ring) that spills less (p1_ring below)
    auto fat_ok = [&](int c, bool sparse) {
        int sc = sparse ? in.scr_sp[c] : in.scr[0][c];
        if (!sparse && in.p1ring && in.scr[1][c] >= 0 && (sc < 0 || in.scr[1][c] < sc)) sc = in.scr[1][c];
        return sc >= 0 && sc <= 64;
    };
    bool use_sp = false;
    if (in.ok && in.fat && in.sp) {
        double best_d = 1e300, best_s = 1e300;
        for (int c = 1; c <= kPNR; ++c) {
            const int rows = kPG * c, n_l = (B + rows - 1) / rows;  // launches of c rows per group
            if (fat_ok(c, false)) best_d = std::min(best_d, n_l * us[c]);
            if (fat_ok(c, true)) best_s = std::min(best_s, n_l * us_sp[c]);
        }
        use_sp = in.force_sp || best_s < best_d;
    }
    if (in.ok) {
        // the options in this order (it decides ties in solve): register-resident by rows per
        // group, wide by rows per group, then the 17 .. 32-row block
        std::vector<Opt> opts;
        if (in.fat) {
            for (int c = 1; c <= kPNR; ++c)
                if (fat_ok(c, use_sp)) opts.push_back({c, false, (use_sp ? us_sp : us)[c]});
        } else {
            for (int r = 1; r <= kPNR; ++r)
                if (in.ok_reg[r]) opts.push_back({r, false, in.gen ? R.gen[r] : R.rr[r]});
        }
        const bool wide_offered = head_ok && in.wmode &&
                                  ((in.wide_scr >= 0 && in.wide_scr <= hd->max_scratch) || in.allow_wide_scratch);
        if (wide_offered) {
            if (in.wmode == 1) opts.clear();
            for (int r = 1; r <= kPWideRows; ++r) opts.push_back({r, true, wide_cost(r)});
        }
        if (in.nr_max > 0) {  // diagnostic: variant A/B (WRNN_PERSIST_NR_MAX)
            const int c = std::max(1, std::min(kPNR, in.nr_max));
            opts.erase(std::remove_if(opts.begin(), opts.end(), [&](const Opt& o) { return o.wide || o.nr != c; }),
                       opts.end());
            if (opts.empty()) opts.push_back({c, false, 1.0});
        }
        // the cheapest sequence of launches from `opts` over the call's rows
        auto solve = [&](const std::vector<Opt>& opts, std::vector<PLaunch>& lplan) {
            // best[r]: cheapest plan for r rows; pick[r]: its first launch
            std::vector<double> best(B + 1, 0.0);
            std::vector<int> pick(B + 1, -1);
            for (int r = 1; r <= B; ++r) {
                best[r] = 1e300;
                for (int o = 0; o < (int)opts.size(); ++o) {
                    const double c = opts[o].us + best[std::max(0, r - kPG * opts[o].nr)];
                    if (c < best[r] - 1e-9) {
                        best[r] = c;
                        pick[r] = o;
                    }
                }
            }
            int rb = 0;
            for (int r = B; r > 0;) {
                const Opt& o = opts[pick[r]];
                lplan.push_back({rb, o.nr, o.wide});
                rb += kPG * o.nr;
                r = std::max(0, r - kPG * o.nr);
            }
            return best[B];
        };
        if (!opts.empty()) out.plan_us = solve(opts, out.lplan);
        // geneing, 32 rows selected: the 32-row ring instances read no stream, so they enter only
        // plans whose launches are all wide -- the cheapest all-wide plan over 1 .. 32 rows per
        // group (launches of at most 16 on the existing instances, by their own keys) replaces the
        // plan above when it is cheaper. The MOL draw stream is padded to the 32-row launch
        if (wide_offered && hd->key32 && in.gen32 && in.nr_max <= 0 && !out.lplan.empty() &&
            (!mol || (double)S * (B + kPG * kPWideGen32Rows) * kMolNoise * 4.0 < 2147483648.0)) {
            const double* k = hd->key32(R);
            std::vector<Opt> wopts;
            for (const Opt& o : opts)
                if (o.wide) wopts.push_back(o);
            for (int r = kPWideRows + 1; r <= kPWideGen32Rows; ++r) wopts.push_back({r, true, k[0] + k[1] * r});
            std::vector<PLaunch> lp32;
            const double us32 = solve(wopts, lp32);
            if (us32 < out.plan_us - 1e-9) {
                out.lplan = std::move(lp32);
                out.plan_us = us32;
            }
        }
    }
    // time-sliced wide launches, when cheaper than the plan above by the same rates (P1 formed
    // in-kernel: the fatchord ring, runtimeracer per frame). geneing: opt-in (gen_slices: the ring
    // can be taken and the sliced instance is within its scratch rule), where the head's wide
    // launches are offered; planned over the rows padded to the 8 groups (padding rows repeat the
    // last real row, as in the plain launches), the MOL draw stream held to the 2 GiB its sliced
    // instance indexes in 32 bits
    const int Bs = in.gen ? kPG * ((B + kPG - 1) / kPG) : B;
    const bool fr_slices = hd && hd->slices && (in.fat ? in.p1ring : in.rr_frames) && in.wide_rot_scr == 0;
    const bool gen_slices = hd && in.gen && in.gen_slices && in.nr_max <= 0 &&
                            ((in.wide_scr >= 0 && in.wide_scr <= hd->max_scratch) || in.allow_wide_scratch) &&
                            (!mol || (double)S * Bs * kMolNoise * 4.0 < 2147483648.0);
    if (head_ok && (fr_slices || gen_slices) && !out.lplan.empty() && !in.slice_off && in.wmode) {
        std::vector<WLaunch> sl;
        if (plan_wide_slices(Bs, S, sl)) {
            double cost = R.slice[0] * (sl.size() - 1);  // (an extra launch: weights, ring prologue)
            // (the geneing slices run on instances of their own: the head's wide_gen_slice* key)
            const double* ks = gen_slices ? hd->key_slice(R) : nullptr;
            for (const auto& L : sl) cost += L.steps * (ks ? ks[0] + ks[1] * L.nr : wide_cost(L.nr));
            if (cost < R.slice[1] * out.plan_us * S) {
                out.lplan.clear();
                for (int j = 0; j < (int)sl.size(); ++j) out.lplan.push_back({0, sl[j].nr, true, j});
                out.wrot = std::move(sl);
            }
        }
    }
    for (auto& L : out.lplan) L.sp = L.wide && wide_is_sp(L.nr);
    const auto& lp = out.lplan;
    // (time-sliced: the rows the slices were planned for -- B itself for fatchord and runtimeracer)
    out.Bplan = lp.empty() ? B : !out.wrot.empty() ? Bs : lp.back().rb + kPG * lp.back().nr;
    // P1 ring (fatchord): on unless a register-resident launch spills more with it than with the
    // stream (MOL at 3 rows per group: one register, 6.87 against 6.53 us per step); the sparse
    // instances exist with the ring only
    out.p1_ring = in.p1ring;
    bool any_reg = false;
    for (const auto& L : lp) any_reg |= !L.wide;
    if (use_sp && any_reg) {
        out.sparse = true;
    } else if (in.fat) {
        for (const auto& L : lp)
            if (out.p1_ring && !L.wide && in.scr[1][L.nr] > in.scr[0][L.nr]) out.p1_ring = false;
    }
    // row rotation: one register-resident launch with uneven groups becomes K launches over
    // rotating row sets. plan_rotation derives its (q + 1)-row body from B, so the launch must
    // run exactly ceil(B / 8) rows per group; every rotated kernel forms its noise offsets in
    // 32 bits, so the padded noise stream must stay below 4 GB
    if (lp.size() != 1 || lp[0].wide || lp[0].nr != (B + kPG - 1) / kPG) return;
    if (!((double)S * out.Bplan * in.n * 4.0 < 4.0e9) || in.rot_off) return;
    if (in.mode != WRNN_MODE_RAW && in.mode != WRNN_MODE_MOL) return;
    const int nr = lp[0].nr;
    const bool fat_rot = in.fat && out.p1_ring && in.cpw <= 16;
    if (nr < 2 || !(fat_rot || in.rr || in.gen)) return;
    const double* u = in.fat  ? (out.sparse ? R.rot9_sp : R.rot9)
                      : in.rr ? (mol ? R.rot_rrm : in.cpw > 16 ? R.rot_rr10 : R.rot_rr9)
                              : (mol ? R.rot_genm : R.rot_gen);
    double t_hi = u[nr], t_lo = u[nr - 1];
    // fatchord MOL: its rotated 3-row body (one spilled register) runs much slower than the 2-row
    // one -- the split balanced for 5.91 / 4.70 is the fastest of a scan (C3 5.61 -> 5.19)
    if (in.fat && mol && nr == 3 && !out.sparse) t_lo = R.rot_mol3_lo;
    if (in.rot_hi > 0 && in.rot_lo > 0) {
        t_hi = in.rot_hi;
        t_lo = in.rot_lo;
    }
    // (the MOL 3-row rotated instance keeps one spilled register: tolerated, §3.0e)
    const int rs = in.scr_rot[out.sparse ? 1 : 0][nr];
    if (rs < 0 || rs > 8) return;
    if (plan_rotation(B, S, t_hi, t_lo, out.rot, R.rot[0], R.rot[1])) {
        out.lplan.clear();
        for (int j = 0; j < out.rot.K; ++j) out.lplan.push_back({0, nr, false, j});
    }
}

// The per-step streams a planned call writes before its launches, and whether the workspace check
// admits the persistent engine. One function for generate_impl (which sets p1_stream / gen_ring
// from it), wrnn_stream_info and wrnn_debug_stream_bytes, so the three cannot drift.
//   P1:    [S][Bp][np] floats unless every launch forms P1 in-kernel (fatchord ring, runtimeracer
//          and geneing calls of wide launches only); then step 0 alone is formed: 0 bytes
//   noise: the extent of the [S][Bp][n] Gumbel (RAW) or [S][Bp][kMolNoise] MOL stream; 0 when every
//          launch draws in-kernel (Beta; RAW calls of in-kernel-noise wide launches only)
// geneing ring (gen_frames: the per-frame P1 form exists and the ring instances run spill-free):
// only calls whose launches are all wide (time-sliced ones are ring instances). sw =
// WRNN_GEN_RING: 1 the ring where possible, 0 the streams, -1 the default -- the ring when the streams would not fit the
// workspace cap, or when the head's measured call time is not above the stream form's
// (kGenRingDefault).
// The cap: fatchord and runtimeracer keep the whole-call bound S Bp (4 H + n) 4 bytes whatever
// they write; geneing counts the streams the call really writes (P1 with its cI column).
constexpr bool kGenRingDefault[3] = {true, true, true};  // BITS, MOL, Beta
StreamPlan plan_streams(const PlanIn& in, const PlanOut& out, bool p1x4, bool gen_frames, int sw) {
    StreamPlan sp;
    const int H = in.fat ? kPH : kRH;
    const double rows_steps = (double)in.S * out.Bplan;
    bool any_wide = false, any_reg = false;
    for (const auto& L : out.lplan) {
        any_wide |= L.wide;
        any_reg |= !L.wide;
    }
    const bool all_wide = any_wide && !any_reg;
    const bool raw = in.mode == WRNN_MODE_RAW;
    sp.p1_stream = !out.p1_ring;
    if (in.rr && in.rr_frames && all_wide) sp.p1_stream = false;  // runtimeracer: only wide launches
    const double p1_full = rows_steps * (p1x4 ? 4 : 3) * H * 4.0;
    const double noise_unit = in.mode == WRNN_MODE_BETA ? 0.0 : raw ? in.n * 4.0 : kMolNoise * 4.0;
    // (persist_noise: RAW calls of fatchord / runtimeracer wide launches only draw in-kernel)
    double noise = raw && all_wide && !in.gen ? 0.0 : rows_steps * noise_unit;
    if (in.gen) {
        const double cap_p1 = rows_steps * 4 * H * 4.0;  // (P1 and cI: 4 H floats either way)
        const bool streams_fit = cap_p1 + noise <= kPersistWsBytes;
        const bool can = gen_frames && all_wide && in.mode >= 0 && in.mode <= 2;
        sp.gen_ring = can && sw != 0 && (sw == 1 || !streams_fit || kGenRingDefault[in.mode]);
        // (a 32-row launch and a time-sliced one exist only as ring instances: plan_call offers them
        // only where `can` holds and the switch is not 0, so their plans always take the ring)
        bool any32 = false;
        for (const auto& L : out.lplan) any32 |= L.wide && L.nr > kPWideRows;
        if (any32 || !out.wrot.empty()) sp.gen_ring = can && sw != 0;
        if (sp.gen_ring) {
            sp.p1_stream = false;
            if (raw) noise = 0.0;  // (MOL keeps its k_mol_noise stream)
        }
        sp.persist_ok = (sp.gen_ring ? 0.0 : cap_p1) + noise <= kPersistWsBytes;
    } else {
        sp.persist_ok = rows_steps * (4 * H + in.n) * 4.0 <= kPersistWsBytes;
    }
    sp.p1_bytes = sp.p1_stream ? p1_full : 0.0;
    sp.noise_bytes = noise;
    return sp;
}

int debug_plan_in(int model_type, int bits, int mode, int rows, int seq_len, int flags, PlanIn& in) {
    if (rows < 1 || seq_len < 1) return fail(WRNN_ERR_INVALID, "bad arguments");
    // (1 << bits below; the planner's tables have rows + 1 entries)
    if (bits < 1 || bits > 10) return fail(WRNN_ERR_INVALID, "bits must be 1..10");
    if (mode != WRNN_MODE_RAW && mode != WRNN_MODE_MOL && mode != WRNN_MODE_BETA)
        return fail(WRNN_ERR_INVALID, "mode must be one of WRNN_MODE_*");
    if (rows > kPlanRowsMax) return fail(WRNN_ERR_INVALID, "rows above " + std::to_string(kPlanRowsMax));
    in = PlanIn();
    in.ok = true;
    in.fat = model_type == WRNN_MODEL_FATCHORD;
    in.rr = model_type == WRNN_MODEL_RUNTIMERACER;
    in.gen = model_type == WRNN_MODEL_GENEING;
    if (!in.fat && !in.rr && !in.gen) return fail(WRNN_ERR_INVALID, "model type");
    in.mode = mode;
    in.n = mode == WRNN_MODE_RAW ? (1 << bits) : mode == WRNN_MODE_BETA ? 2 : 30;
    in.cpw = (in.n + kPM - 1) / kPM;  // (classes per slot, as pack_persist* sets it)
    in.c10 = in.n > kPM * 16;
    in.B = rows;
    in.S = seq_len;
    // flags: 1 sparse image, 2 P1 ring / per-frame P1 (fatchord, runtimeracer), 4 wide images
    // (fatchord RAW / MOL, runtimeracer RAW, geneing BITS with 512 or 1024 classes), 16 the
    // runtimeracer MOL wide image, 32 the geneing MOL wide image, 64 the geneing Beta wide image;
    // every variant spill-free. (128, geneing in-kernel conditioning, enters the plan only through
    // 256: the geneing 32-row ring instances are available and selected -- it needs 128 and the
    // head's flag 4 / 32 / 64; wrnn_debug_stream_bytes); 512 the block-sparse wide image (fatchord
    // RAW, with flag 4); 1024: the geneing time-sliced instances are available and selected (needs
    // 128 and the head's flag, like 256)
    in.sp = in.fat && (flags & 1) && (flags & 2) && (mode == WRNN_MODE_RAW || mode == WRNN_MODE_MOL);
    in.force_sp = in.sp && (flags & 8);
    in.p1ring = in.fat && (flags & 2);
    in.rr_frames = in.rr && (flags & 2);
    const bool raw = mode == WRNN_MODE_RAW, mol = mode == WRNN_MODE_MOL;
    const int head_flag = in.fat ? (raw || mol ? 4 : 0)
                          : in.rr ? (raw ? 4 : mol ? 16 : 0)
                                  : (raw ? (in.n == 512 || in.n == 1024 ? 4 : 0) : mol ? 32 : 64);
    in.has_wide = (flags & head_flag) != 0;
    in.has_wide_sp = (flags & 512) && in.fat && raw && in.has_wide;
    in.gen32 = (flags & 256) && (flags & 128) && in.gen && in.has_wide;
    in.gen_slices = (flags & 1024) && (flags & 128) && in.gen && in.has_wide;
    for (int c = 1; c <= kPNR; ++c) in.ok_reg[c] = true;
    return WRNN_OK;
}

}  // namespace wrnn

using namespace wrnn;

extern "C" {

int wrnn_debug_plan(const char* table, int model_type, int bits, int mode, int rows, int seq_len, int flags,
                    int* n_launches, int* rows_per_group, int* wide, int cap, int* rot_launches) {
    if (!n_launches || !rot_launches) return fail(WRNN_ERR_INVALID, "null argument");
    if (cap < 0) return fail(WRNN_ERR_INVALID, "bad arguments");
    PlanRates R;
    std::string err;
    PlanIn in;
    if (int rc = debug_plan_in(model_type, bits, mode, rows, seq_len, flags, in)) return rc;
    if (table && !parse_rates(table, R, err)) return fail(WRNN_ERR_INVALID, "rate table: " + err);
    PlanOut out;
    plan_call(in, R, out);
    *n_launches = (int)out.lplan.size();
    *rot_launches = out.rot.K;
    for (int i = 0; i < (int)out.lplan.size() && i < cap; ++i) {
        if (rows_per_group) rows_per_group[i] = out.lplan[i].nr;
        if (wide) wide[i] = out.lplan[i].sp ? 2 : out.lplan[i].wide ? 1 : 0;
    }
    return WRNN_OK;
}

int wrnn_debug_stream_bytes(int model_type, int bits, int mode, int rows, int seq_len, int flags,
                            double* p1_bytes, double* noise_bytes, int* persist_ok) {
    if (!p1_bytes || !noise_bytes || !persist_ok) return fail(WRNN_ERR_INVALID, "null argument");
    PlanIn in;
    if (int rc = debug_plan_in(model_type, bits, mode, rows, seq_len, flags, in)) return rc;
    PlanOut out;
    plan_call(in, PlanRates(), out);  // the shipped rates
    // (the x4 P1 form of the shipped models; no switch: the default rule)
    const StreamPlan sp = plan_streams(in, out, true, in.gen && (flags & 128), -1);
    *p1_bytes = sp.p1_bytes;
    *noise_bytes = sp.noise_bytes;
    *persist_ok = !out.lplan.empty() && sp.persist_ok ? 1 : 0;
    return WRNN_OK;
}

int wrnn_debug_rot_plan(int rows, int seq_len, double us_hi, double us_lo, int* launches, int* n_hi,
                        int* n_lo, int* vmap, size_t capacity) {
    if (!launches || !n_hi || !n_lo) return fail(WRNN_ERR_INVALID, "null argument");
    if (rows < 1 || seq_len < 1 || !(us_hi > 0) || !(us_lo > 0)) return fail(WRNN_ERR_INVALID, "bad arguments");
    RotPlan P;
    *launches = *n_hi = *n_lo = 0;
    if (!plan_rotation(rows, seq_len, us_hi, us_lo, P)) return WRNN_OK;
    const int nv = kPG * P.nr_hi;
    if (vmap) {
        if (capacity < (size_t)P.K * nv * 2) return fail(WRNN_ERR_CAPACITY, "capacity");
        for (int j = 0; j < P.K; ++j)
            for (int v = 0; v < nv; ++v) {
                const int g = v % kPG, r = v / kPG;
                const bool used = r < P.gnr[(size_t)j * kPG + g];
                const VRow m = P.vmap[(size_t)j * nv + v];
                vmap[((size_t)j * nv + v) * 2] = used ? m.row : -1;
                vmap[((size_t)j * nv + v) * 2 + 1] = used ? m.off : -1;
            }
    }
    *launches = P.K;
    *n_hi = P.n_hi;
    *n_lo = P.n_lo;
    return WRNN_OK;
}

int wrnn_debug_slice_plan(int rows, int seq_len, int* launches, int* rows_steps, size_t rs_capacity, int* vmap,
                          size_t capacity) {
    if (!launches || !rows_steps) return fail(WRNN_ERR_INVALID, "null argument");
    if (rows < 1 || seq_len < 1) return fail(WRNN_ERR_INVALID, "bad arguments");
    std::vector<WLaunch> sl;
    *launches = 0;
    if (!plan_wide_slices(rows, seq_len, sl)) return WRNN_OK;
    const int K = (int)sl.size(), nv = kPG * kPWideRows;
    if (rs_capacity < 2 * (size_t)K || (vmap && capacity < (size_t)K * nv * 2)) return fail(WRNN_ERR_CAPACITY, "capacity");
    for (int k = 0; k < K; ++k) {
        rows_steps[2 * k] = sl[k].nr;
        rows_steps[2 * k + 1] = sl[k].steps;
        if (vmap)
            for (int v = 0; v < nv; ++v) {
                const bool used = v < kPG * sl[k].nr;
                vmap[((size_t)k * nv + v) * 2] = used ? sl[k].vmap[v].row : -1;
                vmap[((size_t)k * nv + v) * 2 + 1] = used ? sl[k].vmap[v].off : -1;
            }
    }
    *launches = K;
    return WRNN_OK;
}

}  // extern "C"
