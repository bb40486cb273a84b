// Stand-alone check of the block-sparse wide packer (sparse_wide_pack.h) for the ASan + UBSan build
// of `make wide_sp_check`: packs random block-sparse matrices (empty and full slots, rows past the
// matrix, narrow matrices, -0.0 blocks, denormals and NaNs), rebuilds every row from its lists and
// compares it bit for bit; checks the fit rule at both ends of the carve, the two handle-free
// wrnn_debug_wide_sp_* entry points with good and bad arguments, and the planner's use of the
// image (plan.h: flag, rate key, forced and forbidden). Exit status 0: every check held (the
// sanitizers abort the run otherwise).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "plan.h"
#include "sparse_wide_pack.h"
#include "wavernn_mi355x.h"

using namespace wrnn;

namespace {

long g_checks = 0;
#define REQUIRE(cond, ...)                                         \
    do {                                                           \
        ++g_checks;                                                \
        if (!(cond)) {                                             \
            std::fprintf(stderr, "wide_sp_check: %s failed: ", #cond); \
            std::fprintf(stderr, __VA_ARGS__);                     \
            std::fprintf(stderr, "\n");                            \
            std::exit(1);                                          \
        }                                                          \
    } while (0)

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}
float rnd_val() { return ((int)(rnd() % 2001) - 1000) / 512.0f + 1.0f / 4096.0f; }  // never zero

// rows x cols with each 1 x 4 block live with probability keep / 1000; rows in [full_lo, full_hi)
// fully live, rows in [empty_lo, empty_hi) fully dead
std::vector<float> sparse_matrix(int rows, int cols, int keep, int full_lo = 0, int full_hi = 0, int empty_lo = 0,
                                 int empty_hi = 0) {
    std::vector<float> W((size_t)rows * cols, 0.f);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c + 4 <= cols; c += 4) {
            const bool full = r >= full_lo && r < full_hi, empty = r >= empty_lo && r < empty_hi;
            if (empty || (!full && (int)(rnd() % 1000) >= keep)) continue;
            for (int i = 0; i < 4; ++i) W[(size_t)r * cols + c + i] = rnd_val();
            // (a live block may hold zeros: one nonzero word keeps it)
            if (rnd() % 4 == 0) W[(size_t)r * cols + c + rnd() % 4] = 0.f;
        }
    return W;
}

int live_blocks(const float* row, int cols) {
    int n = 0;
    for (int c = 0; c + 4 <= cols; c += 4) {
        uint32_t w[4];
        std::memcpy(w, row + c, sizeof w);
        n += ((w[0] | w[1] | w[2] | w[3]) << 1) != 0u;
    }
    return n;
}

void check_lists(const char* what, const std::vector<float>& W, int rows, int cols, int row0, int nrows) {
    wsp::Lists L;
    REQUIRE(wsp::append_rows(W.data(), rows, cols, cols, row0, nrows, L), "%s: append", what);
    REQUIRE((int)L.start.size() == nrows && (int)L.count.size() == nrows, "%s: row table", what);
    REQUIRE(L.blocks.size() == 4 * L.col.size(), "%s: blocks / columns", what);
    std::vector<float> out(cols);
    int at = 0;
    for (int r = 0; r < nrows; ++r) {
        REQUIRE(L.start[r] == at, "%s: row %d starts at %d, not %d", what, r, L.start[r], at);
        at += L.count[r];
        for (int i = 1; i < L.count[r]; ++i)
            REQUIRE(L.col[L.start[r] + i - 1] < L.col[L.start[r] + i], "%s: row %d not by ascending column", what, r);
        wsp::densify_row(L, r, cols, out.data());
        if (row0 + r < rows) {
            const float* src = W.data() + (size_t)(row0 + r) * cols;
            REQUIRE(L.count[r] == live_blocks(src, cols), "%s: row %d holds %d blocks", what, r, L.count[r]);
            // (-0.0 words of a dead block come back as +0.0: compare those as values, the rest as bits)
            for (int c = 0; c + 4 <= cols; c += 4)
                if (wsp::dead4(src + c))
                    REQUIRE(wsp::dead4(out.data() + c), "%s: row %d block %d revived", what, r, c / 4);
                else
                    REQUIRE(!std::memcmp(src + c, out.data() + c, 16), "%s: row %d block %d differs", what, r, c / 4);
        } else {
            REQUIRE(L.count[r] == 0, "%s: a row past the matrix has blocks", what);
        }
    }
    REQUIRE(at == L.size(), "%s: %d blocks listed of %d", what, at, L.size());
}

struct Model {
    std::vector<float> ih2, hh1, hh2, fc1, fc2, fc3;
    int ld_ih2, ld_fc, n;
    wsp::StepMatrices mats() const {
        return {ih2.data(), hh1.data(), hh2.data(), fc1.data(), fc2.data(), fc3.data(), ld_ih2, kPH, kPH, ld_fc, ld_fc, kPH, n};
    }
};
Model model(int keep, int n) {
    Model m;
    m.ld_ih2 = kPH + 32;
    m.ld_fc = kPH + 32;
    m.n = n;
    m.ih2 = sparse_matrix(3 * kPH, m.ld_ih2, keep);
    m.hh1 = sparse_matrix(3 * kPH, kPH, keep);
    m.hh2 = sparse_matrix(3 * kPH, kPH, keep);
    m.fc1 = sparse_matrix(kPH, m.ld_fc, keep);
    m.fc2 = sparse_matrix(kPH, m.ld_fc, keep);
    m.fc3 = sparse_matrix(n, kPH, keep);
    return m;
}

void check_image(int keep, int n, bool want_fit) {
    const Model m = model(keep, n);
    const wsp::Image im = wsp::build_image(m.mats());
    REQUIRE(im.fits == want_fit, "keep %d n %d: fits %d", keep, n, (int)im.fits);
    REQUIRE(im.total == (long long)(11 * kPH + n) * wsp::kColBlocks, "keep %d n %d: total %lld", keep, n, im.total);
    int fits = -1, fill = -1;
    double dens = -1;
    REQUIRE(wrnn_debug_wide_sp_image(m.ih2.data(), m.ld_ih2, m.hh1.data(), m.hh2.data(), m.fc1.data(), m.ld_fc,
                                     m.fc2.data(), m.ld_fc, m.fc3.data(), n, &fits, &dens, &fill) == WRNN_OK,
            "image entry");
    REQUIRE(fits == (int)im.fits && fill == im.fill_f4 && dens == im.density(), "image entry: outputs");
    if (!want_fit) {
        REQUIRE(im.slots.empty(), "no image keeps no lists");
        return;
    }
    REQUIRE((int)im.slots.size() == wsp::kSlots && im.fill_f4 <= wsp::kCapF4, "fill %d", im.fill_f4);
    long long live = 0;
    std::vector<float> out(kPH);
    for (int w = 0; w < wsp::kSlots; ++w) {
        const wsp::Lists& L = im.slots[w];
        REQUIRE((int)L.start.size() == wsp::kSets * wsp::kRows, "slot %d: rows", w);
        live += L.size();
        // set s, row i of the slot against its matrix row (the x part: the first 512 columns)
        for (int s = 0; s < wsp::kSets; ++s)
            for (int i = 0; i < wsp::kRows; ++i) {
                const int u = wsp::kRows * w + i;
                const float* src = s < wsp::S_HH1    ? &m.ih2[(size_t)(s * kPH + u) * m.ld_ih2]
                                   : s < wsp::S_FC1  ? &m.hh1[(size_t)((s - wsp::S_HH1) * kPH + u) * kPH]
                                   : s == wsp::S_FC1 ? &m.fc1[(size_t)u * m.ld_fc]
                                   : s == wsp::S_FC2 ? &m.fc2[(size_t)u * m.ld_fc]
                                   : s == wsp::S_FC3 ? (u < n ? &m.fc3[(size_t)u * kPH] : nullptr)
                                   : s == wsp::S_FC3B ? (kPH + u < n ? &m.fc3[(size_t)(kPH + u) * kPH] : nullptr)
                                                      : &m.hh2[(size_t)((s - wsp::S_HH2) * kPH + u) * kPH];
                wsp::densify_row(L, s * wsp::kRows + i, kPH, out.data());
                if (src)
                    REQUIRE(!std::memcmp(src, out.data(), kPH * sizeof(float)), "slot %d set %d row %d differs", w, s, i);
                else
                    REQUIRE(L.count[s * wsp::kRows + i] == 0, "slot %d set %d row %d: no such class", w, s, i);
            }
    }
    REQUIRE(live == im.live, "live %lld / %lld", live, im.live);
}

int plan_of(int rows, int S, int bits, int flags, const char* table, std::vector<int>& wide) {
    int n = 0, rot = 0;
    std::vector<int> nr(600);
    wide.assign(600, -1);
    REQUIRE(wrnn_debug_plan(table, WRNN_MODEL_FATCHORD, bits, WRNN_MODE_RAW, rows, S, flags, &n, nr.data(), wide.data(),
                            600, &rot) == WRNN_OK,
            "plan entry");
    wide.resize(n);
    return n;
}

void check_planner() {
    std::vector<int> wd, base;
    // C4 per GPU: 11 time-sliced launches, sparse wide under a cheap key, dense otherwise
    REQUIRE(plan_of(144, 12100, 9, 2 | 4 | 512, "wide_sp 3 0.2 1", wd) == 11, "144 rows: launches");
    for (int x : wd) REQUIRE(x == 2, "144 rows, cheap key: wide = %d", x);
    plan_of(144, 12100, 9, 2 | 4, nullptr, base);
    for (const char* t : {(const char*)nullptr, "wide_sp 30 1 5"}) {
        plan_of(144, 12100, 9, 2 | 4 | 512, t, wd);
        REQUIRE(wd == base, "144 rows, dear or shipped key: the plan without the image");
    }
    plan_of(144, 12100, 9, 2 | 4, "wide_sp 3 0.2 1", wd);
    REQUIRE(wd == base, "144 rows: the key without the image");
    // env WRNN_SPARSE_WIDE as the runtime hands it over (PlanIn::sp_wide_mode)
    PlanIn in;
    REQUIRE(debug_plan_in(WRNN_MODEL_FATCHORD, 9, WRNN_MODE_RAW, 144, 12100, 2 | 4 | 512, in) == WRNN_OK, "plan in");
    PlanRates R, cheap;
    std::string err;
    REQUIRE(parse_rates("wide_sp 3 0.2 1", cheap, err), "%s", err.c_str());
    PlanOut out;
    in.sp_wide_mode = 1;
    plan_call(in, R, out);
    for (const auto& L : out.lplan) REQUIRE(L.wide && L.sp, "forced: every wide launch sparse");
    in.sp_wide_mode = 0;
    plan_call(in, cheap, out);
    for (const auto& L : out.lplan) REQUIRE(L.wide && !L.sp, "forbidden: no sparse launch");
    in.sp_wide_mode = -1;
    in.has_wide_sp = false;
    plan_call(in, cheap, out);
    for (const auto& L : out.lplan) REQUIRE(!L.sp, "no image: no sparse launch");
    // the table round trip carries the key
    PlanRates T;
    REQUIRE(parse_rates(rates_text(cheap).c_str(), T, err) && T.wide_sp[0] == 3 && T.wide_sp[1] == 0.2 && T.wide_sp[2] == 1,
            "round trip");
    for (const char* bad : {"wide_sp 5", "wide_sp 5 0.1", "wide_sp 5 0.1 1 2", "wide_sp 5 x 1", "wide_sp 5 -1 1", "wide_sp 0 1 1"})
        REQUIRE(!parse_rates(bad, T, err), "'%s' accepted", bad);
}

}  // namespace

int main() {
    // lists of one matrix: the three tested shapes, a narrow matrix, rows past the end, an empty and
    // a full slot
    for (int keep : {0, 100, 500, 1000}) {
        const std::vector<float> W = sparse_matrix(1536, 512, keep, 32, 48, 64, 80);
        for (int row0 : {0, 16, 32, 64, 512 + 32, 1024 + 64, 1520, 1530}) check_lists("1536 x 512", W, 1536, 512, row0, 16);
        const std::vector<float> N = sparse_matrix(40, 12, keep);
        check_lists("40 x 12", N, 40, 12, 32, 16);
        check_lists("40 x 12, every row", N, 40, 12, 0, 40);
    }
    {  // special words: -0.0 blocks are dead, a denormal, a NaN or one -0.0 among values keeps the block
        std::vector<float> W(16 * 16, 0.f);
        for (int i = 0; i < 4; ++i) W[i] = -0.0f;
        W[4] = -0.0f;
        W[5] = 1.0f;
        W[8] = std::numeric_limits<float>::denorm_min();
        W[12] = std::numeric_limits<float>::quiet_NaN();
        wsp::Lists L;
        REQUIRE(wsp::append_rows(W.data(), 16, 16, 16, 0, 16, L), "append");
        REQUIRE(L.count[0] == 3 && L.col[0] == 1 && L.col[1] == 2 && L.col[2] == 3, "special words: %d blocks", L.count[0]);
        REQUIRE(!std::memcmp(&L.blocks[0], &W[4], 16) && !std::memcmp(&L.blocks[8], &W[12], 16), "special words kept as bits");
        check_lists("special words", W, 16, 16, 0, 16);
    }
    // the debug entry: outputs, null outputs, bad arguments
    {
        const std::vector<float> W = sparse_matrix(1024, 512, 100);
        std::vector<float> rec(32 * 512);
        std::vector<int> sz(32);
        int tot = -1;
        REQUIRE(wrnn_debug_wide_sp_pack(W.data(), 1024, 512, 31, rec.data(), sz.data(), &tot) == WRNN_OK, "pack entry");
        int sum = 0;
        for (int r = 0; r < 32; ++r) {
            const float* src = &W[(size_t)((r / 16) * 512 + 16 * 31 + r % 16) * 512];
            REQUIRE(!std::memcmp(src, &rec[(size_t)r * 512], 512 * sizeof(float)), "pack entry: row %d", r);
            REQUIRE(sz[r] == live_blocks(src, 512), "pack entry: size of row %d", r);
            sum += sz[r];
        }
        REQUIRE(sum == tot, "pack entry: total");
        REQUIRE(wrnn_debug_wide_sp_pack(W.data(), 1024, 512, 0, nullptr, nullptr, nullptr) == WRNN_OK, "null outputs");
        REQUIRE(wrnn_debug_wide_sp_pack(nullptr, 1024, 512, 0, nullptr, nullptr, nullptr) == WRNN_ERR_INVALID, "null matrix");
        for (int rows : {0, 16, 511, 513, 2048})
            REQUIRE(wrnn_debug_wide_sp_pack(W.data(), rows, 512, 0, nullptr, nullptr, nullptr) == WRNN_ERR_INVALID, "rows %d", rows);
        for (int cols : {0, 3, 510, 516, -4})
            REQUIRE(wrnn_debug_wide_sp_pack(W.data(), 512, cols, 0, nullptr, nullptr, nullptr) == WRNN_ERR_INVALID, "cols %d", cols);
        for (int slot : {-1, 32})
            REQUIRE(wrnn_debug_wide_sp_pack(W.data(), 512, 512, slot, nullptr, nullptr, nullptr) == WRNN_ERR_INVALID, "slot %d", slot);
        REQUIRE(wrnn_debug_wide_sp_image(nullptr, 512, W.data(), W.data(), W.data(), 512, W.data(), 512, W.data(), 512,
                                         nullptr, nullptr, nullptr) == WRNN_ERR_INVALID, "image entry: null matrix");
    }
    // the fit rule: 90 % pruned fits (512, 700 and 1024 classes), 50 % pruned and dense do not; an
    // all-zero model fits with empty lists
    check_image(100, 512, true);
    check_image(100, 1024, true);
    check_image(100, 700, true);
    check_image(0, 1024, true);
    check_image(500, 512, false);
    check_image(1000, 1024, false);
    check_planner();
    std::printf("wide_sp_check: %ld checks held\n", g_checks);
    return 0;
}
