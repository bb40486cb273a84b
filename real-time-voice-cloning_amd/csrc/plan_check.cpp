// Stand-alone check of the launch planner (plan.h) for the ASan + UBSan build of `make plan_check`:
// walks the plan grid of tools/plan_dump.py natively and asserts the invariants of every plan, feeds
// parse_rates well- and ill-formed tables, and calls the handle-free wrnn_debug_* entry points with
// bad arguments. Exit status 0: every check held (the sanitizers abort the run otherwise).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "plan.h"
#include "wavernn_mi355x.h"

using namespace wrnn;

namespace {

long g_checks = 0;
#define REQUIRE(cond, ...)                                     \
    do {                                                       \
        ++g_checks;                                            \
        if (!(cond)) {                                         \
            std::fprintf(stderr, "plan_check: %s failed: ", #cond); \
            std::fprintf(stderr, __VA_ARGS__);                 \
            std::fprintf(stderr, "\n");                        \
            std::exit(1);                                      \
        }                                                      \
    } while (0)

struct Head {
    const char* name;
    int model, bits, mode;
};
const Head kHeads[] = {
    {"fat_raw9", WRNN_MODEL_FATCHORD, 9, WRNN_MODE_RAW},      {"fat_raw10", WRNN_MODEL_FATCHORD, 10, WRNN_MODE_RAW},
    {"fat_mol", WRNN_MODEL_FATCHORD, 9, WRNN_MODE_MOL},       {"rr_raw9", WRNN_MODEL_RUNTIMERACER, 9, WRNN_MODE_RAW},
    {"rr_raw10", WRNN_MODEL_RUNTIMERACER, 10, WRNN_MODE_RAW}, {"rr_mol", WRNN_MODEL_RUNTIMERACER, 9, WRNN_MODE_MOL},
    {"gen_raw9", WRNN_MODEL_GENEING, 9, WRNN_MODE_RAW},       {"gen_raw10", WRNN_MODEL_GENEING, 10, WRNN_MODE_RAW},
    {"gen_mol", WRNN_MODEL_GENEING, 9, WRNN_MODE_MOL},        {"gen_beta", WRNN_MODEL_GENEING, 9, WRNN_MODE_BETA},
};
const int kSeq[] = {63, 64, 1200, 6000, 12100, 14000};

// every subset of the flag bits the topology reads, and all nine bits
std::vector<int> flag_sets(int model) {
    const std::vector<int> bits = model == WRNN_MODEL_FATCHORD       ? std::vector<int>{1, 2, 4, 8}
                                  : model == WRNN_MODEL_RUNTIMERACER ? std::vector<int>{2, 4, 16}
                                                                     : std::vector<int>{4, 32, 64, 128, 256, 1024};
    std::vector<int> sets;
    for (int s = 0; s < (1 << bits.size()); ++s) {
        int f = 0;
        for (size_t i = 0; i < bits.size(); ++i)
            if (s >> i & 1) f |= bits[i];
        sets.push_back(f);
    }
    sets.push_back(511);
    return sets;
}

// every physical row of a rotated / time-sliced plan runs exactly S steps, each launch from the
// step its earlier launches left it at
void check_maps(const Head& h, const PlanIn& in, const PlanOut& out) {
    // (geneing slices are planned for the rows padded to the 8 groups: the padding rows run too)
    const int nrows = std::max(in.B, out.wrot.empty() ? 0 : out.Bplan);
    std::vector<long> done(nrows, 0);
    auto take = [&](const VRow& v, int steps) {
        REQUIRE(v.row >= 0 && v.row < nrows, "%s rows %d: mapped row %d", h.name, in.B, v.row);
        REQUIRE(v.off == done[v.row], "%s rows %d: row %d starts at %d after %ld steps", h.name, in.B, v.row, v.off,
                done[v.row]);
        done[v.row] += steps;
    };
    if (!out.wrot.empty()) {
        REQUIRE(out.wrot.size() == out.lplan.size(), "%s rows %d: slices / launches", h.name, in.B);
        for (const auto& L : out.wrot) {
            REQUIRE(L.nr >= 1 && L.nr <= kPWideRows && L.steps >= 1 && L.vmap.size() == (size_t)kPG * L.nr,
                    "%s rows %d: slice of %d rows, %d steps", h.name, in.B, L.nr, L.steps);
            for (const auto& v : L.vmap) take(v, L.steps);
        }
    } else {
        const RotPlan& P = out.rot;
        REQUIRE(P.K == (int)out.lplan.size() && P.nr_hi >= 2 && P.nr_hi <= kPNR, "%s rows %d: rotation", h.name, in.B);
        const size_t nv = (size_t)kPG * P.nr_hi;
        REQUIRE(P.vmap.size() == P.K * nv && P.gnr.size() == (size_t)P.K * kPG && P.git.size() == P.gnr.size(),
                "%s rows %d: rotation tables", h.name, in.B);
        for (int j = 0; j < P.K; ++j)
            for (int g = 0; g < kPG; ++g) {
                const int nr = P.gnr[(size_t)j * kPG + g], it = P.git[(size_t)j * kPG + g];
                REQUIRE((nr == P.nr_hi && it == P.n_hi) || (nr == P.nr_hi - 1 && it == P.n_lo),
                        "%s rows %d: group of %d rows, %d steps", h.name, in.B, nr, it);
                for (int r = 0; r < nr; ++r) take(P.vmap[j * nv + g + (size_t)kPG * r], it);
            }
    }
    for (int r = 0; r < nrows; ++r) REQUIRE(done[r] == in.S, "%s rows %d: row %d ran %ld steps", h.name, in.B, r, done[r]);
}

void check_plan(const Head& h, int rows, int S, int flags) {
    PlanIn in;
    REQUIRE(debug_plan_in(h.model, h.bits, h.mode, rows, S, flags, in) == WRNN_OK, "%s rows %d", h.name, rows);
    PlanOut out;
    plan_call(in, PlanRates(), out);
    const auto& lp = out.lplan;
    REQUIRE(!lp.empty(), "%s rows %d S %d flags %d: no plan", h.name, rows, S, flags);
    bool all_wide = true, mapped = lp[0].rot >= 0;
    int rb = 0;
    for (size_t i = 0; i < lp.size(); ++i) {
        const PLaunch& L = lp[i];
        all_wide &= L.wide;
        REQUIRE(L.nr >= 1 && L.nr <= (L.wide ? kPWideGen32Rows : kPNR), "%s rows %d: launch of %d rows per group",
                h.name, rows, L.nr);
        REQUIRE((L.rot >= 0) == mapped, "%s rows %d: mapped and plain launches mixed", h.name, rows);
        if (mapped) {
            REQUIRE(L.rot == (int)i && L.rb == 0, "%s rows %d: mapped launch %zu", h.name, rows, i);
        } else {  // plain launches cover rows 0 .. Bplan back to back
            REQUIRE(L.rb == rb, "%s rows %d: launch %zu starts at row %d, not %d", h.name, rows, i, L.rb, rb);
            rb += kPG * L.nr;
        }
    }
    for (const auto& L : lp)
        REQUIRE(L.nr <= kPWideRows || (in.gen && all_wide), "%s rows %d: %d rows per group outside an all-wide geneing plan",
                h.name, rows, L.nr);
    if (!mapped) REQUIRE(out.Bplan == rb, "%s rows %d: Bplan %d, launches end at %d", h.name, rows, out.Bplan, rb);
    REQUIRE(out.Bplan >= rows, "%s rows %d: Bplan %d", h.name, rows, out.Bplan);
    if (!out.wrot.empty())  // sliced: the rows themselves; geneing pads them to the 8 groups
        REQUIRE(out.Bplan == (in.gen ? kPG * ((rows + kPG - 1) / kPG) : rows), "%s rows %d: sliced for %d rows", h.name, rows,
                out.Bplan);
    REQUIRE(mapped == (!out.wrot.empty() || out.rot.K > 0) && !(out.rot.K > 0 && !out.wrot.empty()),
            "%s rows %d: maps without mapped launches", h.name, rows);
    if (mapped) check_maps(h, in, out);
    // the streams: persist_ok is the answer the reported bytes give
    for (int sw = -1; sw <= 1; ++sw) {
        const StreamPlan sp = plan_streams(in, out, true, in.gen && (flags & 128), sw);
        const double rows_steps = (double)S * out.Bplan;
        REQUIRE(sp.p1_bytes >= 0 && sp.noise_bytes >= 0 && (sp.p1_bytes > 0) == sp.p1_stream, "%s rows %d: bytes", h.name,
                rows);
        if (in.gen)  // (geneing counts what the call writes: the x4 P1 form is its P1 + cI cap)
            REQUIRE(sp.persist_ok == (sp.p1_bytes + sp.noise_bytes <= kPersistWsBytes), "%s rows %d S %d: persist_ok %d",
                    h.name, rows, S, sp.persist_ok);
        else  // (the whole-call bound, which covers whatever is written)
            REQUIRE(sp.persist_ok == (rows_steps * (4 * (in.fat ? kPH : kRH) + in.n) * 4.0 <= kPersistWsBytes) &&
                        (!sp.persist_ok || sp.p1_bytes + sp.noise_bytes <= kPersistWsBytes),
                    "%s rows %d S %d: persist_ok %d", h.name, rows, S, sp.persist_ok);
        // (the ring: all-wide geneing plans, plain or time-sliced, never a rotation; a sliced plan
        // always takes it unless the switch forbids it)
        REQUIRE(!sp.gen_ring || (in.gen && all_wide && out.rot.K == 0 && sw != 0 && !sp.p1_stream), "%s rows %d: ring",
                h.name, rows);
        REQUIRE(!(in.gen && !out.wrot.empty() && sw != 0) || sp.gen_ring, "%s rows %d: slices without the ring", h.name, rows);
    }
}

// a table is taken or refused with a reason; a taken one prints, parses back to itself and plans
void check_table(const std::string& text, int want = -1) {
    PlanRates R;
    std::string err;
    const bool ok = parse_rates(text.c_str(), R, err);
    REQUIRE(ok == err.empty(), "table '%.40s': ok %d, error '%s'", text.c_str(), ok, err.c_str());
    if (want >= 0) REQUIRE(ok == (want != 0), "table '%.40s': ok %d (%s)", text.c_str(), ok, err.c_str());
    if (!ok) return;
    PlanRates T;
    REQUIRE(parse_rates(rates_text(R).c_str(), T, err) && rates_text(T) == rates_text(R), "table '%.40s': round trip",
            text.c_str());
    PlanOut out;  // and it plans
    PlanIn in;
    REQUIRE(debug_plan_in(WRNN_MODEL_FATCHORD, 9, WRNN_MODE_RAW, 144, 12100, 6, in) == WRNN_OK, "plan input");
    plan_call(in, R, out);
    REQUIRE(!out.lplan.empty(), "table '%.40s': no plan", text.c_str());
}

void check_tables() {
    const std::string shipped = rates_text(PlanRates());
    check_table(shipped, 1);
    // every truncation of the shipped table inside one of its lines
    for (size_t cut = 0; cut < shipped.size(); ++cut) check_table(shipped.substr(0, cut));
    check_table("", 1);
    std::string comments;
    for (int i = 0; i < 10000; ++i) comments += "# comment " + std::to_string(i) + "\n";
    check_table(comments, 1);
    check_table(comments + "fat9 1 2 3", 0);
    check_table("fat9 1 2 3 4 5", 0);
    check_table("fat9 1 2 3", 0);
    check_table("rot_mol3_lo", 0);
    check_table("rot_mol3_lo 4.7 4.7", 0);
    check_table("wide 1 2", 0);
    check_table("fat9 1 2 3 x", 0);
    check_table("fat9 x", 0);
    check_table("fat9 0 1 2 3", 0);
    check_table("fat9 1 2 3 0", 0);
    check_table("wide 1 -2 3", 0);
    check_table("fat9 1 2 3 nan", 0);
    check_table("fat9 nan nan nan nan", 0);
    check_table("fat9 1 2 3 1e400", 0);
    check_table("fat9 1e400 1 2 3");  // (how the stream reads an overflow is the library's; no crash, no inf)
    check_table("fat9 1 2 3 4 1e400");
    check_table("nosuchkey 1 2", 0);
    check_table("wid 1 2 3", 0);
    check_table("wide_gen3 1 2", 0);
    // a key that is a prefix of another names itself only
    PlanRates R;
    std::string err;
    REQUIRE(parse_rates("wide 1 2 3\n", R, err) && R.wide[0] == 1 && R.wide[2] == 3 &&
                R.wide_gen32[0] == PlanRates().wide_gen32[0] && R.wide_gen[1] == PlanRates().wide_gen[1],
            "key 'wide'");
    R = PlanRates();
    REQUIRE(parse_rates("wide_gen32 7 8\n", R, err) && R.wide_gen32[0] == 7 && R.wide_gen32[1] == 8 &&
                R.wide[0] == PlanRates().wide[0] && R.wide_gen[0] == PlanRates().wide_gen[0] &&
                R.wide_gen32_mol[0] == PlanRates().wide_gen32_mol[0],
            "key 'wide_gen32'");
    // the register-resident tables keep slot 0 and take rows per group 1..4
    R = PlanRates();
    REQUIRE(parse_rates("gen 1 2 3 4\n", R, err) && R.gen[0] == 0 && R.gen[1] == 1 && R.gen[4] == 4 && R.wide_gen[0] == 3.508,
            "key 'gen'");
}

void check_entry_points() {
    const int F = WRNN_MODEL_FATCHORD, RAW = WRNN_MODE_RAW;
    int n = -7, rot = -7;
    std::vector<int> nr(3, -7), wd(3, -7);
    REQUIRE(wrnn_debug_plan(nullptr, F, 9, RAW, 18, 12100, 6, nullptr, nr.data(), wd.data(), 3, &rot) == WRNN_ERR_INVALID, "null n");
    REQUIRE(wrnn_debug_plan(nullptr, F, 9, RAW, 18, 12100, 6, &n, nr.data(), wd.data(), 3, nullptr) == WRNN_ERR_INVALID, "null rot");
    REQUIRE(wrnn_debug_plan(nullptr, F, 9, RAW, 18, 12100, 6, &n, nullptr, nullptr, 3, &rot) == WRNN_OK && n == 3 && rot == 3,
            "null arrays");
    REQUIRE(wrnn_debug_plan(nullptr, F, 9, RAW, 18, 12100, 6, &n, nr.data(), wd.data(), -1, &rot) == WRNN_ERR_INVALID, "cap -1");
    REQUIRE(wrnn_debug_plan(nullptr, F, 9, RAW, 18, 12100, 6, &n, nr.data(), wd.data(), 0, &rot) == WRNN_OK && n == 3 &&
                nr[0] == -7 && wd[0] == -7,
            "cap 0");
    REQUIRE(wrnn_debug_plan(nullptr, F, 9, RAW, 18, 12100, 6, &n, nr.data(), wd.data(), 2, &rot) == WRNN_OK && n == 3 &&
                nr[1] == 3 && nr[2] == -7 && wd[2] == -7,
            "cap one short");
    for (int bits : {0, 11})
        REQUIRE(wrnn_debug_plan(nullptr, F, bits, RAW, 18, 12100, 6, &n, nr.data(), wd.data(), 3, &rot) == WRNN_ERR_INVALID,
                "bits %d", bits);
    for (int rows : {0, kPlanRowsMax + 1})
        REQUIRE(wrnn_debug_plan(nullptr, F, 9, RAW, rows, 12100, 6, &n, nr.data(), wd.data(), 3, &rot) == WRNN_ERR_INVALID,
                "rows %d", rows);
    REQUIRE(wrnn_debug_plan(nullptr, F, 9, RAW, 18, 0, 6, &n, nr.data(), wd.data(), 3, &rot) == WRNN_ERR_INVALID, "seq_len 0");
    REQUIRE(wrnn_debug_plan(nullptr, 3, 9, RAW, 18, 12100, 6, &n, nr.data(), wd.data(), 3, &rot) == WRNN_ERR_INVALID, "model");
    REQUIRE(wrnn_debug_plan(nullptr, F, 9, 3, 18, 12100, 6, &n, nr.data(), wd.data(), 3, &rot) == WRNN_ERR_INVALID, "mode");
    REQUIRE(wrnn_debug_plan("fat9 1", F, 9, RAW, 18, 12100, 6, &n, nr.data(), wd.data(), 3, &rot) == WRNN_ERR_INVALID &&
                std::string(wrnn_last_error()) == "rate table: line 1: 'fat9' takes 4 values",
            "bad table: %s", wrnn_last_error());

    double p1 = -1, nz = -1;
    int ok = -7;
    REQUIRE(wrnn_debug_stream_bytes(F, 9, RAW, 18, 12100, 6, nullptr, &nz, &ok) == WRNN_ERR_INVALID, "null p1");
    REQUIRE(wrnn_debug_stream_bytes(F, 9, RAW, 18, 12100, 6, &p1, nullptr, &ok) == WRNN_ERR_INVALID, "null noise");
    REQUIRE(wrnn_debug_stream_bytes(F, 9, RAW, 18, 12100, 6, &p1, &nz, nullptr) == WRNN_ERR_INVALID, "null ok");
    for (int bits : {0, 11}) REQUIRE(wrnn_debug_stream_bytes(F, bits, RAW, 18, 12100, 6, &p1, &nz, &ok) == WRNN_ERR_INVALID, "bits");
    for (int rows : {0, kPlanRowsMax + 1})
        REQUIRE(wrnn_debug_stream_bytes(F, 9, RAW, rows, 12100, 6, &p1, &nz, &ok) == WRNN_ERR_INVALID, "rows");
    REQUIRE(wrnn_debug_stream_bytes(F, 9, RAW, 18, 12100, 6, &p1, &nz, &ok) == WRNN_OK && ok == 1 && p1 == 0 && nz > 0, "C2 streams");

    int k = -7, nh = -7, nl = -7;
    const size_t need = 3 * 8 * 3 * 2;  // C2: 3 launches of 3 rows per group
    std::vector<int> vm(need - 1, -7);
    REQUIRE(wrnn_debug_rot_plan(18, 12100, 5.91, 5.22, nullptr, &nh, &nl, nullptr, 0) == WRNN_ERR_INVALID, "null launches");
    REQUIRE(wrnn_debug_rot_plan(18, 12100, 5.91, 5.22, &k, nullptr, &nl, nullptr, 0) == WRNN_ERR_INVALID, "null n_hi");
    REQUIRE(wrnn_debug_rot_plan(18, 12100, 5.91, 5.22, &k, &nh, nullptr, nullptr, 0) == WRNN_ERR_INVALID, "null n_lo");
    REQUIRE(wrnn_debug_rot_plan(0, 12100, 5.91, 5.22, &k, &nh, &nl, nullptr, 0) == WRNN_ERR_INVALID, "rows 0");
    REQUIRE(wrnn_debug_rot_plan(18, 0, 5.91, 5.22, &k, &nh, &nl, nullptr, 0) == WRNN_ERR_INVALID, "seq_len 0");
    REQUIRE(wrnn_debug_rot_plan(18, 12100, 0, 5.22, &k, &nh, &nl, nullptr, 0) == WRNN_ERR_INVALID, "us 0");
    REQUIRE(wrnn_debug_rot_plan(18, 12100, 5.91, std::nan(""), &k, &nh, &nl, nullptr, 0) == WRNN_ERR_INVALID, "us nan");
    REQUIRE(wrnn_debug_rot_plan(18, 12100, 5.91, 5.22, &k, &nh, &nl, nullptr, 0) == WRNN_OK && k == 3, "no map");
    REQUIRE(wrnn_debug_rot_plan(18, 12100, 5.91, 5.22, &k, &nh, &nl, vm.data(), 0) == WRNN_ERR_CAPACITY, "capacity 0");
    REQUIRE(wrnn_debug_rot_plan(18, 12100, 5.91, 5.22, &k, &nh, &nl, vm.data(), need - 1) == WRNN_ERR_CAPACITY && vm[0] == -7,
            "capacity one short");
    REQUIRE(wrnn_debug_rot_plan(kPlanRowsMax + 1, 12100, 5.91, 5.22, &k, &nh, &nl, vm.data(), need - 1) == WRNN_OK && k == 0,
            "rows beyond any rotation");

    const size_t K = 11, need_rs = 2 * K, need_vm = K * 8 * 16 * 2;  // C4: 9 + 2 launches
    std::vector<int> rs(need_rs - 1, -7), svm(need_vm - 1, -7);
    REQUIRE(wrnn_debug_slice_plan(144, 12100, nullptr, rs.data(), rs.size(), nullptr, 0) == WRNN_ERR_INVALID, "null launches");
    REQUIRE(wrnn_debug_slice_plan(144, 12100, &k, nullptr, 0, nullptr, 0) == WRNN_ERR_INVALID, "null rows_steps");
    REQUIRE(wrnn_debug_slice_plan(0, 12100, &k, rs.data(), rs.size(), nullptr, 0) == WRNN_ERR_INVALID, "rows 0");
    REQUIRE(wrnn_debug_slice_plan(144, 0, &k, rs.data(), rs.size(), nullptr, 0) == WRNN_ERR_INVALID, "seq_len 0");
    REQUIRE(wrnn_debug_slice_plan(144, 12100, &k, rs.data(), 0, nullptr, 0) == WRNN_ERR_CAPACITY, "rs capacity 0");
    REQUIRE(wrnn_debug_slice_plan(144, 12100, &k, rs.data(), need_rs - 1, nullptr, 0) == WRNN_ERR_CAPACITY && rs[0] == -7,
            "rs capacity one short");
    std::vector<int> rs_ok(need_rs, -7);
    REQUIRE(wrnn_debug_slice_plan(144, 12100, &k, rs_ok.data(), need_rs, svm.data(), need_vm - 1) == WRNN_ERR_CAPACITY &&
                rs_ok[0] == -7 && svm[0] == -7,
            "map capacity one short");
    REQUIRE(wrnn_debug_slice_plan(144, 12100, &k, rs_ok.data(), need_rs, nullptr, 0) == WRNN_OK && k == (int)K && rs_ok[0] == 16,
            "C4 slices");
    REQUIRE(wrnn_debug_slice_plan(kPlanRowsMax + 1, 12100, &k, rs.data(), 0, nullptr, 0) == WRNN_OK && k == 0, "rows beyond any slicing");
}

}  // namespace

int main() {
    std::vector<int> rows;
    for (int r = 1; r <= 72; ++r) rows.push_back(r);
    for (int r : {131, 144, 152, 232, 360, 2115, 4096}) rows.push_back(r);
    long plans = 0;
    for (const Head& h : kHeads)
        for (int flags : flag_sets(h.model))
            for (int r : rows)
                for (int S : kSeq) {
                    check_plan(h, r, S, flags);
                    ++plans;
                }
    // the stand-alone rotation and slice plans of the dump
    for (int r = 136; r <= 512; r += 8)
        for (int S : kSeq) {
            std::vector<WLaunch> sl;
            if (!plan_wide_slices(r, S, sl)) continue;
            PlanIn in;
            in.B = r;
            in.S = S;
            PlanOut out;
            out.wrot = sl;
            out.lplan.resize(sl.size());
            check_maps(Head{"slices", 0, 0, 0}, in, out);
        }
    check_tables();
    check_entry_points();
    std::printf("plan_check: %ld plans, %ld checks held\n", plans, g_checks);
    return 0;
}
