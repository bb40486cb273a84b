// Host runtime of the MI355X WaveRNN vocoder: weight packing, workspace, the per-step stage
// program, HIP-graph capture of the recurrence, and the extern "C" ABI of
// include/wavernn_mi355x.h.
//
// Reference behaviour restated here (paths in RuntimeRacer/Real-Time-Voice-Cloning):
//   generate()            vocoder/models/fatchord_version.py:155-240, runtimeracer_version.py:199-295
//   pad/upsample          fatchord_version.py:170-172, :60-85
//   fold_with_overlap     fatchord_version.py:290-340 (never materialised: rows index positions)
//   load_state_dict names vocoder/inference.py:35 / base.py:18-109 topologies
//   loadWeights/melToWav  vocoder/libwavernn/<variant>/src/WaveRNNVocoder.cpp:22-47 (errors, seed)
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "cand_key.h"
#include "philox.h"
#include "plan.h"
#include "sparse_wide_pack.h"
#include "wavernn_mi355x.h"
#include "wrnn_kernels.h"

using namespace wrnn;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPC(x)                                                                             \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess)                                                               \
            return fail(WRNN_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_));      \
    } while (0)

#define CHECK(x)                         \
    do {                                 \
        int rc_ = (x);                   \
        if (rc_ != WRNN_OK) return rc_;  \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    int alloc(size_t n) {
        if (n <= bytes && p) return WRNN_OK;
        release();
        if (n == 0) n = 16;
        hipError_t e = hipMalloc(&p, n);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(WRNN_ERR_OOM, "hipMalloc(" + std::to_string(n) + "): " +
                                          hipGetErrorString(e));
        }
        bytes = n;
        return WRNN_OK;
    }
    float* f() const { return (float*)p; }
};

struct PackedSeg {
    std::shared_ptr<DevBuf> W;
    int cfg = 0, n_out = 0, n_tiles = 0, K = 0;
};

// one matvec segment of a stage, in terms of named per-row slots
enum Slot {
    SL_NONE = -1,
    SL_X1 = 0, SL_X2, SL_X3, SL_X4,
    SL_Y1, SL_Y2, SL_Y3, SL_Y4,
    SL_H1, SL_H2, SL_H3, SL_H4,
    SL_GH1, SL_GH2, SL_GH3, SL_GH4,
    SL_P1, SL_LOG,
    SL_CI,  // gather from per-position cI at step t+1
    SL_COUNT
};

struct SegDesc {
    PackedSeg w;
    int kind;
    int x;          // Slot
    int y;          // Slot (EPI_BIAS3 / EPI_COND*)
    const float* cond;  // constant device vector (c_ld == 0) ...
    int c_ld;       // ... or -1: per-frame conditioning at column fcol of ws.fcond
    int fcol;
    int gh, h, xout;  // EPI_GRU slots
};

struct StageDesc {
    std::string name;
    int K;
    std::vector<SegDesc> segs;
    bool next_step_only;  // segment list index 1.. may be dropped at the last step (P1)
};

}  // namespace

struct wrnn_handle {
    wrnn_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    // PERSIST: the noise is generated on a side stream while the upsample / conditioning
    // GEMMs run on `stream` (independent inputs); the recurrence waits on noise_done
    hipStream_t side = nullptr;
    hipEvent_t rows_ready = nullptr, noise_done = nullptr;
    bool noise_pending = false;
    int H = 0, F = 0, A = 0, C = 0, R = 0, n_classes = 0, feat = 0, hop = 0, n_gru = 0, KI = 0;
    int indent = 0;
    std::map<std::string, std::vector<int64_t>> expected;
    std::map<std::string, std::vector<float>> host;
    bool finalized = false;
    uint64_t seed = 0;
    uint32_t stream_ctr = 0;
    std::vector<uint32_t> utt_streams;  // wrnn_set_utt_streams: explicit streams of the next call
    std::vector<int> fold_lo, fold_hi;  // wrnn_set_fold_ranges: fold rows of the next batch call
    // teacher-forced logit gate (wrnn_set_debug_steps): the steps to record, the device map
    // [S] step -> slot and the capture [kDbgSteps][Bp][n] of the last call; dbg_gen keys the
    // captured CHAIN graphs (their k_sample arguments hold the buffers)
    std::vector<int> dbg_steps;
    DevBuf dbg_out, dbg_map;
    uint64_t dbg_gen = 0;  // its own graph-key field (no shifted int: ADVICE r3)
    int dbg_rows = 0, dbg_S = 0;
    DbgLogits dbg{};

    // ---- device weights
    std::vector<std::shared_ptr<DevBuf>> wbufs;
    const float* Wci = nullptr;               // conv_in (C, feat*ksz)
    const float *bn_a = nullptr, *bn_b = nullptr;  // (1 + 2*res_blocks) x C alpha / beta
    std::vector<const float*> Wres;           // 2*res_blocks x (C, C)
    const float *Wco = nullptr, *bco = nullptr;
    std::vector<const float*> upk;            // up-layer kernels
    const float *WIT = nullptr, *bI = nullptr, *w0 = nullptr, *v1 = nullptr;
    struct AuxCond {
        int slice;          // aux slice index (1..3)
        const float* WT;    // (A, n_out)
        const float* bias;  // (n_out)
        int n_out;
        int offset;         // column offset inside the per-frame cond row
    };
    std::vector<AuxCond> auxc;
    int cond_width = 0;
    std::map<std::string, const float*> dvec;  // constant vectors (biases)
    std::vector<StageDesc> stages;

    // ---- workspace (capacity keyed on rows/steps)
    struct Workspace {
        int B = 0, S = 0, Pcap = 0, Fcap = 0, Tcap = 0, Ncap = 0;
        int N = 0;  // frame columns of the MelResNet activations of the last call (sum of T)
        DevBuf slots[SL_COUNT];
        DevBuf labels, samples, noise, cI, fcond, rows, stamps;
        DevBuf mel_in, act0, act1, Rb, up1, up2, melup;
        DevBuf q4, a4;  // per-frame P1 projections [1 + T][np] (slot 0 = zero frame)
        size_t mel_in_cap = 0;
    } ws;
    // captured recurrence chunks: (t0, len, S if last chunk else -1, rows, timing, MOL seed)
    std::map<std::tuple<int, int, int, int, int, uint64_t, uint64_t>, hipGraphExec_t> graphs;

    // ---- call state
    int last_B = 0, last_S = 0, last_L0 = 0, last_T0 = 0;
    bool melup_valid = false;  // ws.melup holds the last call's upsampled mel (not per-frame P1)
    bool p1_ring = false;      // this call's k_persist launches form P1 in-kernel
    bool p1_stream = false;    // this call writes the [S][B][4H] P1 stream (other kernels)
    bool gen_ring = false;     // geneing: every launch is wide and forms P1 / the noise in-kernel
    int gen_wide_rows = kPWideRows;  // wrnn_set_gen_wide_rows: 16, or 32 (the 32-row ring instances)
    bool gen_wide_slices = false;    // wrnn_set_gen_wide_slices: geneing time-sliced wide launches
    double last_p1_bytes = 0, last_noise_bytes = 0;  // the per-step streams of the last call (wrnn_stream_info)
    bool sparse_call = false;  // this call's k_persist launches run the sparse instances
    bool sparse_wide_call = false;  // a launch of this call ran the block-sparse wide kernel
    PlanRates rates;           // per-step rates of the launch planner (load_rates, §3.0h)
    bool timing = false;
    int phase_step = -1;  // diagnostic (env WRNN_PHASE_STEP): per-phase stamps of one step
    DevBuf phases;
    std::vector<double> stage_avg_us;
    std::vector<int> stage_launches;
    int nrt = 1, RT = 4;
    int nrg = 2;  // row groups per stage tile (env WRNN_NRG: 1, 2 or 4)
    std::vector<RowInfo> rows_host;

    // ---- persistent engine (kernels_persist.hip)
    struct PersistW {
        bool ok = false;  // weights packed (fatchord 512 / runtimeracer 256 dims, n <= 1024)
        bool rr = false;  // runtimeracer topology (kernels_persist_rr.hip)
        bool gen = false; // geneing topology (kernels_persist_gen.hip)
        int cpw = 0, nw = 0, oG2 = 0, oF1 = 0, oF2 = 0;  // rr: oG2 = oG3, oF2 = oF3
        const float *wreg = nullptr, *wlds = nullptr;
        const float *M1T = nullptr, *bP1 = nullptr;  // P1 straight from the conditioning input
        bool p1x4 = false;  // fatchord: P1 as [step][row][unit][r, z, n, cI] (one 16-B load)
        // P1 from per-frame projections + the upsampler's per-phase taps (pack_p1)
        bool p1taps_ok = false;
        const float *p1taps = nullptr, *zero_np = nullptr;
        int p1split = -1;  // phase from which the 4 in-kernel taps start at frame f - 1
        const float *wwide = nullptr, *wwide_lds = nullptr;  // wide-row launches (MFMA images)
        const float* wfc3b = nullptr;  // ... > 512 classes: the second fc3 tile (L2-streamed)
        const float* wwide_rr = nullptr;  // runtimeracer wide-row launches (kernels_persist_wide_rr.hip)
        const float* wwide_gen = nullptr;  // geneing BITS / MOL / Beta wide-row launches (kernels_persist_wide_gen.hip)
        // sparse k_persist image (pruned checkpoints, pack_persist_sparse):
        // per-lane masks / list bases [kPM][kPT] uint4 and the block lists [kPM][kPLdsW4] float4
        bool sp_ok = false;
        // block-sparse wide image (pack_persist_wide_sp; kernels_persist_wide_sp.hip): null when
        // the lists do not fit; the live fraction and the fullest slot's blocks either way
        const float* wsp_img = nullptr;
        double wsp_density = 0;
        int wsp_fill = 0;
        const float *swreg = nullptr, *swlds = nullptr;
        double sp_density = 1.0;   // live fraction of the kernel's 1 x 4 weight blocks
        int sp_fill = 0;           // float4 of the fullest slot's lists (of kPSpZero)
        double sp_live_bytes = 0;  // live step-weight bytes (blocks x 16 B + a 2-byte index each)
        double sp_live_macs = 0;   // live MACs per row-step of the pruned step matrices
        const float *b_hh1 = nullptr, *b_hh2 = nullptr, *b_fc3 = nullptr;  // rr: b_fc3 = fc5 bias
        const float *b_ih2 = nullptr, *b_ih4 = nullptr, *b_hh3 = nullptr, *b_hh4 = nullptr,
                    *b_f2 = nullptr, *b_f4 = nullptr;  // rr only
    } pw;
    struct PersistWS {
        DevBuf P1, gumbel, ctl, xbuf, st, stamps, phases, wring, rot;
    } pws;
    int engine = WRNN_ENGINE_AUTO;  // requested engine (wrnn_set_engine / env WRNN_ENGINE)
    int last_engine = WRNN_ENGINE_CHAIN;
    bool persist_failed = false;    // kPersistMaxStreak persistent calls in a row failed: CHAIN
    int persist_fail_streak = 0;    // consecutive persistent calls that fell back
    int fallbacks = 0;              // calls on this handle that fell back PERSIST -> CHAIN
    std::string fallback_reason;    // why the last one did
    unsigned* prog_host = nullptr;  // host-mapped progress word (kernels publish steps done)
    unsigned* prog_dev = nullptr;
    int last_Bp = 0;                // rows the last call ran (padded to 8 * rows-per-group)
    RotPlan rot_plan;               // row rotation of the last call (plan.h)
    std::vector<WLaunch> wrot;      // time-sliced wide launches of the last call (§3.0f)
    std::vector<PLaunch> p_plan;    // PERSIST: the launches of the last call, in order
    std::vector<int> pev_kind;      // per timed launch: 1 wide, 0 otherwise
    std::vector<int> pev_rows;      // per timed launch: rows (8 nr)
    std::vector<hipEvent_t> pev;    // PERSIST timing events (start, end) per launch
    std::vector<double> pev_steps;
    std::vector<char> rot_host;     // the row rotation's per-launch tables (uploaded per call)
    double p_step_bytes = 0, p_step_flops = 0;  // algorithmic per step
    double p_wbytes = 0, p_row_bytes = 0, p_macs = 0;  // per step: weights, per row-step, MACs/row
    struct PStage {
        std::string name;  // "persist" (register-resident kernels) or "persist_wide"
        int wide;
        double rows;       // real rows summed over the kind's launches
        int launches;
        double steps = 0, row_steps = 0;  // steps / real row-steps summed over the kind's launches
    };
    std::vector<PStage> pstages;  // launch kinds of the last PERSIST call
    double p_avg_steps = 0;                      // steps per timed launch
    // ---- streaming sessions (stream.hip): the open sessions, the per-launch group table
    std::vector<struct wrnn_stream*> sessions;
    DevBuf stream_tab;

    ~wrnn_handle() {
        for (auto e : pev) (void)hipEventDestroy(e);
        for (auto& kv : graphs) (void)hipGraphExecDestroy(kv.second);
        if (rows_ready) (void)hipEventDestroy(rows_ready);
        if (noise_done) (void)hipEventDestroy(noise_done);
        if (prog_host) (void)hipHostFree(prog_host);
        if (side) (void)hipStreamDestroy(side);
        if (stream) (void)hipStreamDestroy(stream);
    }

    float* slot(int s) const { return ws.slots[s].f(); }
    int slot_width(int s) const {
        switch (s) {
            case SL_X1: case SL_X2: case SL_X3: case SL_X4:
            case SL_H1: case SL_H2: case SL_H3: case SL_H4: return H;
            case SL_Y1: case SL_Y2: case SL_Y3: case SL_Y4: return F;
            case SL_GH1: case SL_GH2: case SL_GH3: case SL_GH4: case SL_P1: return 3 * H;
            case SL_LOG: return n_classes;
            default: return 0;
        }
    }
};

namespace {

std::vector<int64_t> shp(std::initializer_list<int64_t> l) { return std::vector<int64_t>(l); }

void build_expected(wrnn_handle* h) {
    auto& e = h->expected;
    const int C = h->C, R = h->R, H = h->H, F = h->F, A = h->A, n = h->n_classes;
    const int k = h->cfg.pad * 2 + 1;
    e["upsample.resnet.conv_in.weight"] = shp({C, h->feat, k});
    auto bn = [&](const std::string& p) {
        for (const char* f : {"weight", "bias", "running_mean", "running_var"})
            e[p + "." + f] = shp({C});
    };
    bn("upsample.resnet.batch_norm");
    for (int i = 0; i < h->cfg.res_blocks; ++i) {
        const std::string p = "upsample.resnet.layers." + std::to_string(i);
        e[p + ".conv1.weight"] = shp({C, C, 1});
        e[p + ".conv2.weight"] = shp({C, C, 1});
        bn(p + ".batch_norm1");
        bn(p + ".batch_norm2");
    }
    e["upsample.resnet.conv_out.weight"] = shp({R, C, 1});
    e["upsample.resnet.conv_out.bias"] = shp({R});
    for (int j = 0; j < h->cfg.n_upsample; ++j)
        e["upsample.up_layers." + std::to_string(2 * j + 1) + ".weight"] =
            shp({1, 1, 1, 2 * h->cfg.upsample_factors[j] + 1});
    e["I.weight"] = shp({H, h->feat + A});
    e["I.bias"] = shp({H});
    auto gru = [&](const std::string& nm, int inp) {
        e[nm + ".weight_ih_l0"] = shp({3 * H, inp});
        e[nm + ".weight_hh_l0"] = shp({3 * H, H});
        e[nm + ".bias_ih_l0"] = shp({3 * H});
        e[nm + ".bias_hh_l0"] = shp({3 * H});
    };
    auto lin = [&](const std::string& nm, int inp, int out) {
        e[nm + ".weight"] = shp({out, inp});
        e[nm + ".bias"] = shp({out});
    };
    if (h->cfg.model_type == WRNN_MODEL_FATCHORD) {
        gru("rnn1", H);
        gru("rnn2", H + A);
        lin("fc1", H + A, F);
        lin("fc2", F + A, F);
        lin("fc3", F, n);
    } else if (h->cfg.model_type == WRNN_MODEL_GENEING) {  // geneing_version.py:111-114
        gru("rnn1", H);
        lin("fc1", H + A, F);
        lin("fc3", F, n);
    } else {
        gru("rnn1", H);
        gru("rnn2", H);
        gru("rnn3", H + A);
        gru("rnn4", H);
        lin("fc1", H + A, F);
        lin("fc2", F, F);
        lin("fc3", F + A, F);
        lin("fc4", F, F);
        lin("fc5", F, n);
    }
}

// upload a host float vector; returns device pointer kept alive by h->wbufs
const float* upload(wrnn_handle* h, const std::vector<float>& v, int* rc) {
    auto b = std::make_shared<DevBuf>();
    *rc = b->alloc(v.size() * sizeof(float));
    if (*rc) return nullptr;
    hipError_t e = hipMemcpy(b->p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        *rc = fail(WRNN_ERR_HIP, std::string("hipMemcpy weights: ") + hipGetErrorString(e));
        return nullptr;
    }
    h->wbufs.push_back(b);
    return b->f();
}

// Pack rows of a PyTorch (n_rows, ld) weight for the stage tile scheme of kernels_step.hip:
// [tile][kc][og][j][kk] with KC = 256 / (NOG * NRG); TILE_GATE tiles are unit-interleaved
// (j = gate r/z/n of unit u, rows j*H + u of the PyTorch gate-major weight).
PackedSeg pack_segment(wrnn_handle* h, const std::vector<float>& W, int n_out, int ld, int col0,
                       int K, int cfg, int Hg, int* rc) {
    PackedSeg ps;
    ps.cfg = cfg;
    ps.K = K;
    ps.n_out = n_out;
    const int OPL = tile_opl(cfg), NOG = kTileNOG;
    const int KC = kThreads / (NOG * h->nrg), KR = K / KC;
    ps.n_tiles = cfg == TILE_GATE ? (Hg + NOG - 1) / NOG : (n_out + NOG - 1) / NOG;
    std::vector<float> out((size_t)ps.n_tiles * KC * NOG * OPL * KR, 0.f);
    size_t idx = 0;
    for (int tile = 0; tile < ps.n_tiles; ++tile)
        for (int kc = 0; kc < KC; ++kc)
            for (int og = 0; og < NOG; ++og) {
            for (int j = 0; j < OPL; ++j)
                for (int kk = 0; kk < KR; ++kk, ++idx) {
                    int o;
                    bool valid;
                    if (cfg == TILE_GATE) {
                        const int u = tile * NOG + og;
                        valid = u < Hg;
                        o = j * Hg + u;
                    } else {
                        o = tile * NOG + og;
                        valid = o < n_out;
                    }
                    const int k = kc * KR + kk;
                    out[idx] = valid ? W[(size_t)o * ld + col0 + k] : 0.f;
                }
        }
    auto b = std::make_shared<DevBuf>();
    *rc = b->alloc(out.size() * sizeof(float));
    if (*rc) return ps;
    hipError_t e = hipMemcpy(b->p, out.data(), out.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) *rc = fail(WRNN_ERR_HIP, "hipMemcpy packed segment");
    ps.W = b;
    return ps;
}

std::vector<float> transpose_cols(const std::vector<float>& W, int rows, int ld, int col0,
                                  int ncols) {
    // returns (ncols, rows): out[k][o] = W[o][col0 + k]
    std::vector<float> out((size_t)ncols * rows);
    for (int k = 0; k < ncols; ++k)
        for (int o = 0; o < rows; ++o) out[(size_t)k * rows + o] = W[(size_t)o * ld + col0 + k];
    return out;
}

// Persistent-engine weight layout (kernels_persist.hip). Slot w of a group, thread tid
// (og = tid / 16, kc = tid % 16, unit u = 16 w + og % 16) holds in registers, float4 i:
//   0..23  gate j = i / 8 of unit u, k-float4 16 (i % 8) + kc: W_ih2[:, :512] (og < 16) or
//          W_hh1 (og >= 16)
//   24..31 fc2 row u (og < 16) or fc1 row u (og >= 16), x part only
//   32..39 fc3 row cpw w + og when a slot owns more than 16 classes
// and in LDS: W_hh2 rows [16 units][3 gates][128 float4], then fc3 rows [16][128 float4].
// P1 = W_ih1 (I[:,1:] c + b_I) + b_ih1 = M1 c + bP1 with M1 = W_ih1 I[:,1:] (f64 products):
// one K = feat + A - 1 contraction per (step, row) instead of K = rnn_dims (both topologies
// feed rnn1 with I(x0), fatchord_version.py:198-201, runtimeracer_version.py:248-252)
int pack_p1(wrnn_handle* h, bool x4) {
    auto& T = h->host;
    auto& P = h->pw;
    const int H = h->H, A = h->A;
    int rc = WRNN_OK;
    {
        const auto& Wih1 = T["rnn1.weight_ih_l0"];  // (3H, H)
        const auto& WI = T["I.weight"];             // (H, feat + A)
        const auto& bI = T["I.bias"];
        const auto& bih1 = T["rnn1.bias_ih_l0"];
        const int ldI = h->feat + A, KI = h->KI;
        std::vector<double> WIk((size_t)H * KI);
        for (int j = 0; j < H; ++j)
            for (int k = 0; k < KI; ++k) WIk[(size_t)j * KI + k] = WI[(size_t)j * ldI + 1 + k];
        std::vector<float> M1T((size_t)KI * 3 * H), bP1(3 * H);
        std::vector<double> acc(KI);
        for (int o = 0; o < 3 * H; ++o) {
            std::fill(acc.begin(), acc.end(), 0.0);
            double b = bih1[o];
            for (int j = 0; j < H; ++j) {
                const double wv = Wih1[(size_t)o * H + j];
                const double* row = &WIk[(size_t)j * KI];
                for (int k = 0; k < KI; ++k) acc[k] += wv * row[k];
                b += wv * (double)bI[j];
            }
            for (int k = 0; k < KI; ++k) M1T[(size_t)k * 3 * H + o] = (float)acc[k];
            bP1[o] = (float)b;
        }
        P.p1x4 = x4;
        if (x4) {  // columns unit-major, 4 per unit: gates r, z, n of P1, then cI (I.weight)
            std::vector<float> M4((size_t)KI * 4 * H), b4(4 * H);
            for (int k = 0; k < KI; ++k)
                for (int j = 0; j < H; ++j) {
                    for (int g = 0; g < 3; ++g)
                        M4[(size_t)k * 4 * H + 4 * j + g] = M1T[(size_t)k * 3 * H + g * H + j];
                    M4[(size_t)k * 4 * H + 4 * j + 3] = (float)WIk[(size_t)j * KI + k];
                }
            for (int j = 0; j < H; ++j) {
                for (int g = 0; g < 3; ++g) b4[4 * j + g] = bP1[g * H + j];
                b4[4 * j + 3] = bI[j];
            }
            M1T.swap(M4);
            bP1.swap(b4);
        }
        P.M1T = upload(h, M1T, &rc);
        CHECK(rc);
        P.bP1 = upload(h, bP1, &rc);
        CHECK(rc);
        P.zero_np = upload(h, std::vector<float>(bP1.size(), 0.f), &rc);
        CHECK(rc);
    }
    // Per-frame form of P1 (persistent engines): the mel upsampler (fatchord_version.py:47-85)
    // is linear, and for every real frame its response is the same kernel shifted by hop (the
    // `pad` zero frames keep it clear of the sequence ends), so
    //   mel_up(hop f + s) = sum_k K[s][k] mel(f - 2 + k),  k < 5,
    //   P1(p) = M1 [mel_up(p); aux(f)] + bP1 = sum_k K[s][k] Q(f - 2 + k) + Aq(f),
    // Q = M1_mel mel and Aq = M1_aux aux + bP1 per FRAME (two K = 80 / 31 GEMMs over T frames)
    // instead of one K = 111 GEMM per (step, row) over the upsampled mel. K comes from the
    // reference's own stencil chain run on unit impulses in float64 and is checked on every
    // frame of a test sequence; a chain that does not have this form keeps the GEMM path.
    P.p1taps_ok = false;
    {
        const int nu = h->cfg.n_upsample, pad = h->cfg.pad, hop = h->hop, Tt = 9;
        std::vector<std::vector<double>> resp(Tt);
        bool ok = nu >= 1 && hop > 0;
        for (int j = 0; j < Tt && ok; ++j) {
            std::vector<double> cur(Tt, 0.0);
            cur[j] = 1.0;
            int in_pad = pad, T_in = Tt, W_in = Tt + 2 * pad;
            for (int st = 0; st < nu; ++st) {  // k_mel_stencil in float64
                const int s = h->cfg.upsample_factors[st];
                const auto it = T.find("upsample.up_layers." + std::to_string(2 * st + 1) + ".weight");
                if (it == T.end() || (int)it->second.size() != 2 * s + 1) {
                    ok = false;
                    break;
                }
                const auto& wk = it->second;
                const int W_out = W_in * s;
                const bool last = st == nu - 1;
                const int lo = last ? h->indent : 0, len = last ? W_out - 2 * h->indent : W_out;
                std::vector<double> out(len > 0 ? len : 0, 0.0);
                for (int oo = 0; oo < len; ++oo)
                    for (int d = 0; d <= 2 * s; ++d) {
                        const int i = lo + oo + d - s;
                        const int q = (i >= 0 && i < W_out) ? i / s - in_pad : -1;
                        if (q >= 0 && q < T_in) out[oo] += (double)wk[d] * cur[q];
                    }
                cur.swap(out);
                in_pad = 0;
                T_in = W_in = len;
            }
            if ((int)cur.size() != hop * Tt) ok = false;
            resp[j] = std::move(cur);
        }
        // kernel G(x) = response of frame jm at hop jm + x; taps must lie in frames f-2 .. f+2
        std::vector<float> taps((size_t)hop * 8, 0.f);
        if (ok) {
            const int jm = Tt / 2;
            auto G = [&](int x) {
                const int p = hop * jm + x;
                return (p >= 0 && p < hop * Tt) ? resp[jm][p] : 0.0;
            };
            for (int p = 0; p < hop * Tt && ok; ++p) {  // support inside [-2 hop, 3 hop)
                const int x = p - hop * jm;
                if (G(x) != 0.0 && (x < -2 * hop || x >= 3 * hop)) ok = false;
            }
            for (int j = 0; j < Tt && ok; ++j)  // shift invariance on every frame, edges included
                for (int p = 0; p < hop * Tt && ok; ++p) {
                    const double a = resp[j][p], b = G(p - hop * j);
                    if (std::fabs(a - b) > 1e-12 * (1.0 + std::fabs(b))) ok = false;
                }
            // mel_up(hop f + s) = sum_e G(s + hop e) mel(f - e); k = 2 - e
            for (int s = 0; s < hop && ok; ++s)
                for (int k = 0; k < 5; ++k) taps[(size_t)s * 8 + k] = (float)G(s + hop * (2 - k));
        }
        // the in-kernel form (k_persist P1 ring) reads 4 taps: k0 .. k0 + 3 with k0 = 0 below
        // phase `split` and 1 from it on (tap 4 is zero below, tap 0 zero from it on); the
        // sums are the same fma chains, zero taps adding nothing
        int split = -1;
        for (int c = 0; c <= hop && ok && split < 0; ++c) {
            bool good = true;
            for (int s = 0; s < hop && good; ++s)
                good = taps[(size_t)s * 8 + (s < c ? 4 : 0)] == 0.f;
            if (good) split = c;
        }
        if (ok) {
            std::vector<float> all = taps;  // [hop][8] then [hop][4]
            all.resize((size_t)hop * 12, 0.f);
            for (int s = 0; split >= 0 && s < hop; ++s)
                for (int i = 0; i < 4; ++i) all[(size_t)hop * 8 + s * 4 + i] = taps[(size_t)s * 8 + (s >= split) + i];
            P.p1taps = upload(h, all, &rc);
            CHECK(rc);
            P.p1taps_ok = true;
            P.p1split = split;  // -1: no 4-tap form, the stream is used
        }
    }
    return WRNN_OK;
}

int pack_persist_wide(wrnn_handle* h);
int pack_persist_wide_sp(wrnn_handle* h);
int pack_persist_wide_rr(wrnn_handle* h);
int pack_persist_wide_gen(wrnn_handle* h);

int pack_persist_sparse(wrnn_handle* h);

int pack_persist(wrnn_handle* h, int oG2, int oF1, int oF2) {
    auto& T = h->host;
    const int H = h->H, F = h->F, A = h->A, n = h->n_classes;
    auto& P = h->pw;
    P.ok = false;
    P.rr = false;
    P.gen = false;
    if (h->cfg.model_type != WRNN_MODEL_FATCHORD || H != kPH || F != kPH || n > kPM * kPCls)
        return WRNN_OK;
    const auto& Wih2 = T["rnn2.weight_ih_l0"];  // (3H, H + A)
    const auto& Whh1 = T["rnn1.weight_hh_l0"];  // (3H, H)
    const auto& Whh2 = T["rnn2.weight_hh_l0"];  // (3H, H)
    const auto& Wf1 = T["fc1.weight"];          // (F, H + A)
    const auto& Wf2 = T["fc2.weight"];          // (F, F + A)
    const auto& Wf3 = T["fc3.weight"];          // (n, F)
    P.cpw = (n + kPM - 1) / kPM;
    P.nw = persist_reg_f4(P.cpw);
    const int nw = P.nw;
    std::vector<float> wreg((size_t)kPM * kPT * nw * 4, 0.f);
    std::vector<float> wlds((size_t)kPM * kPLdsW4 * 4, 0.f);
    auto put4 = [](float* d, const float* s) { std::memcpy(d, s, 4 * sizeof(float)); };
    for (int w = 0; w < kPM; ++w) {
        for (int tid = 0; tid < kPT; ++tid) {
            const int og = tid >> 4, kc = tid & 15, u = 16 * w + (og & 15);
            float* d = wreg.data() + ((size_t)w * kPT + tid) * nw * 4;
            for (int i = 0; i < 24; ++i) {
                const int j = i / 8, k0 = 4 * (16 * (i % 8) + kc), row = j * H + u;
                put4(d + 4 * i, og < 16 ? &Wih2[(size_t)row * (H + A) + k0] : &Whh1[(size_t)row * H + k0]);
            }
            for (int i = 24; i < 32; ++i) {
                const int k0 = 4 * (16 * (i - 24) + kc);
                put4(d + 4 * i, og < 16 ? &Wf2[(size_t)u * (F + A) + k0] : &Wf1[(size_t)u * (H + A) + k0]);
            }
            if (nw > 32) {
                const int c = P.cpw * w + og;
                if (og < P.cpw && c < n)
                    for (int i = 32; i < 40; ++i)
                        put4(d + 4 * i, &Wf3[(size_t)c * F + 4 * (16 * (i - 32) + kc)]);
            }
        }
        float* L = wlds.data() + (size_t)w * kPLdsW4 * 4;
        for (int ul = 0; ul < 16; ++ul)
            for (int j = 0; j < 3; ++j)
                std::memcpy(L + ((size_t)(ul * 3 + j) * kPK4) * 4,
                            &Whh2[(size_t)(j * H + 16 * w + ul) * H], H * sizeof(float));
        if (P.cpw <= 16)
            for (int og = 0; og < P.cpw; ++og) {
                const int c = P.cpw * w + og;
                if (c < n)
                    std::memcpy(L + ((size_t)16 * 3 * kPK4 + (size_t)og * kPK4) * 4,
                                &Wf3[(size_t)c * F], F * sizeof(float));
            }
    }
    int rc = WRNN_OK;
    P.wreg = upload(h, wreg, &rc);
    CHECK(rc);
    P.wlds = upload(h, wlds, &rc);
    CHECK(rc);
    CHECK(pack_p1(h, true));
    CHECK(pack_persist_wide(h));
    CHECK(pack_persist_wide_sp(h));
    auto dv = [&](const std::string& key) -> const float* {
        if (!h->dvec.count(key)) h->dvec[key] = upload(h, T[key], &rc);
        return h->dvec[key];
    };
    P.b_hh1 = dv("rnn1.bias_hh_l0");
    P.b_hh2 = dv("rnn2.bias_hh_l0");
    P.b_fc3 = dv("fc3.bias");
    CHECK(rc);
    P.oG2 = oG2;
    P.oF1 = oF1;
    P.oF2 = oF2;
    P.ok = true;
    return pack_persist_sparse(h);
}

// Sparse image of the fatchord step weights (kernels_persist.hip sp_products).
// A pruned checkpoint (vocoder/pruner.py:60-88: 1 x 4 column groups zeroed, prune_layers at
// fatchord_version.py:115) carries its masks as zeros; this finds the live blocks of every
// product a k_persist lane owns -- the blocks of its dense register / LDS float4 -- and lists
// them per (product set, 16-lane row group), entry e of lane kc at base + 16 e:
//   A  (mask bits 8 j + q): og < 16 W_ih2[:, :512] rows j H + u, og >= 16 W_hh1 rows j H + u
//   F  (8 bits): og < 16 fc2 row u, og >= 16 fc1 row u          (x parts)
//   H  (24 bits): W_hh2 rows j H + 16 w + (og & 15) -- both halves of the workgroup read the
//      same list (hops B / C / D split its rows, not its weights)
//   C  (8 bits): fc3 class cpw w + og, og < cpw
// with q the dense kernel's block index (columns 4 (16 q + kc) .. + 3). The image exists when
// every slot's lists fit kPSpZero float4 (90 %-pruned fatchord: 6,272, the lists padded to each
// row group's fullest lane); otherwise the dense kernels run the zeros (same results).
int pack_persist_sparse(wrnn_handle* h) {
    auto& T = h->host;
    auto& P = h->pw;
    P.sp_ok = false;
    P.swreg = P.swlds = nullptr;
    P.sp_density = 1.0;
    P.sp_fill = 0;
    const int H = h->H, F = h->F, A = h->A, n = h->n_classes, cpw = P.cpw;
    const auto& Wih2 = T["rnn2.weight_ih_l0"];
    const auto& Whh1 = T["rnn1.weight_hh_l0"];
    const auto& Whh2 = T["rnn2.weight_hh_l0"];
    const auto& Wf1 = T["fc1.weight"];
    const auto& Wf2 = T["fc2.weight"];
    const auto& Wf3 = T["fc3.weight"];
    auto zero4 = [](const float* p) { return p[0] == 0.f && p[1] == 0.f && p[2] == 0.f && p[3] == 0.f; };
    {  // live fraction of the step matrices' 1 x 4 blocks (reported with or without an image)
        long long lv = 0, tot = 0;
        auto scan = [&](const std::vector<float>& W, int rows, int ld) {
            for (int r = 0; r < rows; ++r)
                for (int c = 0; c < kPH; c += 4, ++tot) lv += !zero4(&W[(size_t)r * ld + c]);
        };
        scan(Wih2, 3 * H, H + A);
        scan(Whh1, 3 * H, H);
        scan(Whh2, 3 * H, H);
        scan(Wf1, F, H + A);
        scan(Wf2, F, F + A);
        scan(Wf3, n, F);
        P.sp_density = tot ? (double)lv / (double)tot : 1.0;
    }
    // the block (row pointer, column block q of lane kc) of each set
    auto blkA = [&](int w, int og, int kc, int j, int q) -> const float* {
        const int u = 16 * w + (og & 15), row = j * H + u, k0 = 4 * (16 * q + kc);
        return og < 16 ? &Wih2[(size_t)row * (H + A) + k0] : &Whh1[(size_t)row * H + k0];
    };
    auto blkF = [&](int w, int og, int kc, int q) -> const float* {
        const int u = 16 * w + (og & 15), k0 = 4 * (16 * q + kc);
        return og < 16 ? &Wf2[(size_t)u * (F + A) + k0] : &Wf1[(size_t)u * (H + A) + k0];
    };
    auto blkH = [&](int w, int ul, int kc, int j, int q) -> const float* {
        return &Whh2[(size_t)(j * H + 16 * w + ul) * H + 4 * (16 * q + kc)];
    };
    auto blkC = [&](int w, int og, int kc, int q) -> const float* {
        return &Wf3[(size_t)(cpw * w + og) * F + 4 * (16 * q + kc)];
    };
    std::vector<uint32_t> info((size_t)kPM * kPT * 4, 0u);
    std::vector<float> img((size_t)kPM * kPLdsW4 * 4, 0.f);
    long long live = 0, total = 0;
    double live_macs = 0;
    for (int w = 0; w < kPM; ++w) {
        float* L = img.data() + (size_t)w * kPLdsW4 * 4;
        int top = 0;  // float4 used in this slot
        // one set: per row group og (16 lanes), the lanes' masks, then the lists at `top`
        auto put_set = [&](int og_lo, int og_hi, int nbits, auto blk, int word, int shift, int bword, int bshift,
                           int row_groups_ok) {
            for (int og = og_lo; og < og_hi; ++og) {
                if (!row_groups_ok) continue;
                uint32_t mk[16];
                int cap = 0;
                for (int kc = 0; kc < 16; ++kc) {
                    uint32_t m = 0;
                    for (int b = 0; b < nbits; ++b) {
                        ++total;
                        if (!zero4(blk(og, kc, b))) {
                            m |= 1u << b;
                            ++live;
                        }
                    }
                    mk[kc] = m;
                    cap = std::max(cap, __builtin_popcount(m));
                }
                if (top + 16 * cap > kPSpZero) return false;
                for (int kc = 0; kc < 16; ++kc) {
                    int e = 0;
                    for (int b = 0; b < nbits; ++b)
                        if (mk[kc] >> b & 1u) std::memcpy(L + ((size_t)top + 16 * e++ + kc) * 4, blk(og, kc, b), 16);
                    const int tid = og * 16 + kc;
                    uint32_t* in = &info[((size_t)w * kPT + tid) * 4];
                    in[word] |= mk[kc] << shift;
                    in[bword] |= (uint32_t)(top + kc) << bshift;
                    if (word == 1 && shift == 0) {  // H: the other half of the workgroup reads it too
                        uint32_t* in2 = &info[((size_t)w * kPT + tid + 256) * 4];
                        in2[word] |= mk[kc] << shift;
                        in2[bword] |= (uint32_t)(top + kc) << bshift;
                    }
                }
                top += 16 * cap;
            }
            return true;
        };
        bool ok = put_set(0, 32, 24, [&](int og, int kc, int b) { return blkA(w, og, kc, b / 8, b % 8); }, 0, 0, 2, 0, 1) &&
                  put_set(0, 32, 8, [&](int og, int kc, int b) { return blkF(w, og, kc, b); }, 0, 24, 2, 16, 1) &&
                  put_set(0, 16, 24, [&](int og, int kc, int b) { return blkH(w, og, kc, b / 8, b % 8); }, 1, 0, 3, 0, 1);
        if (ok)
            for (int og = 0; og < std::min(cpw, 32) && ok; ++og)
                ok = put_set(og, og + 1, 8, [&](int o, int kc, int b) { return blkC(w, o, kc, b); }, 1, 24, 3, 16,
                             cpw * w + og < n);
        if (!ok) return WRNN_OK;  // a slot's lists exceed the LDS carve: dense kernels only
        P.sp_fill = std::max(P.sp_fill, top);
    }
    // live MACs per row-step of the pruned step matrices the kernel multiplies (x parts; the aux
    // parts and I are in the per-frame / conditioning GEMMs)
    live_macs = 4.0 * (double)live;
    (void)total;
    P.sp_live_macs = live_macs;
    P.sp_live_bytes = (double)live * 18.0;
    int rc = WRNN_OK;
    std::vector<float> infof(info.size());  // (the words' bits, moved as bytes)
    std::memcpy(infof.data(), info.data(), info.size() * sizeof(uint32_t));
    P.swreg = upload(h, infof, &rc);
    CHECK(rc);
    P.swlds = upload(h, img, &rc);
    CHECK(rc);
    P.sp_ok = true;
    return WRNN_OK;
}

// Wide-row launch weight images (kernels_persist_wide.hip): MFMA A operands. Slot w, wave v,
// lane l, tile T, k-step ks: W_T[row 16 w + (l & 15)][unit 64 v + 16 (l >> 4) + ks]; registers
// [w][v][40 float4 (4 T + ks / 4)][64 l] for T = W_ih2[:, :512] r, z, n | W_hh1 r, z, n | fc1 |
// fc2 | fc3 (x parts only), LDS [w][3 T][v][4 q][64 l][4] for W_hh2 r, z, n; above 512 classes
// the second fc3 tile (rows 512 + 16 w + i) as [w][v][4 q][64 l] float4, read per step. MOL: the
// 30 fc3 rows fill slots 0 and 1 of the same fc3 tile layout (rows u >= n are zero).
int pack_persist_wide(wrnn_handle* h) {
    auto& T = h->host;
    auto& P = h->pw;
    P.wwide = P.wwide_lds = P.wfc3b = nullptr;
    const int H = h->H, F = h->F, A = h->A, n = h->n_classes;
    const bool raw = h->cfg.mode == WRNN_MODE_RAW, mol = h->cfg.mode == WRNN_MODE_MOL && n <= 32;
    if (!(raw || mol) || n > 2 * kPM * 16 || H != kPH || F != kPH) return WRNN_OK;
    const auto& Wih2 = T["rnn2.weight_ih_l0"];  // (3H, H + A)
    const auto& Whh1 = T["rnn1.weight_hh_l0"];  // (3H, H)
    const auto& Whh2 = T["rnn2.weight_hh_l0"];  // (3H, H)
    const auto& Wf1 = T["fc1.weight"];          // (F, H + A)
    const auto& Wf2 = T["fc2.weight"];          // (F, F + A)
    const auto& Wf3 = T["fc3.weight"];          // (n, F)
    auto elem = [&](int w, int t, int i, int k) -> float {
        const int u = 16 * w + i;
        switch (t) {
            case 0: case 1: case 2: return Wih2[(size_t)(t * H + u) * (H + A) + k];
            case 3: case 4: case 5: return Whh1[(size_t)((t - 3) * H + u) * H + k];
            case 6: return Wf1[(size_t)u * (H + A) + k];
            case 7: return Wf2[(size_t)u * (F + A) + k];
            case 8: return u < n ? Wf3[(size_t)u * F + k] : 0.f;
            default: return Whh2[(size_t)((t - 9) * H + u) * H + k];  // 9, 10, 11: r, z, n
        }
    };
    std::vector<float> wr(persist_wide_wreg_floats()), wl(persist_wide_wlds_floats());
    const int nq = (int)(wr.size() / ((size_t)kPM * 8 * 64 * 4));  // float4 per lane (40)
    for (int w = 0; w < kPM; ++w)
        for (int v = 0; v < 8; ++v)
            for (int l = 0; l < 64; ++l) {
                for (int q = 0; q < nq; ++q)
                    for (int c = 0; c < 4; ++c) {
                        const int t = q / 4, ks = 4 * (q % 4) + c;
                        wr[((((size_t)w * 8 + v) * nq + q) * 64 + l) * 4 + c] =
                            elem(w, t, l & 15, 64 * v + 16 * (l >> 4) + ks);
                    }
                for (int t = 0; t < 3; ++t)
                    for (int q = 0; q < 4; ++q)
                        for (int c = 0; c < 4; ++c)
                            wl[(((((size_t)w * 3 + t) * 8 + v) * 4 + q) * 64 + l) * 4 + c] =
                                elem(w, 9 + t, l & 15, 64 * v + 16 * (l >> 4) + 4 * q + c);
            }
    int rc = WRNN_OK;
    if (n > kPM * 16) {
        std::vector<float> wb((size_t)kPM * 8 * 4 * 64 * 4);
        for (int w = 0; w < kPM; ++w)
            for (int v = 0; v < 8; ++v)
                for (int q = 0; q < 4; ++q)
                    for (int l = 0; l < 64; ++l)
                        for (int c = 0; c < 4; ++c) {
                            const int u = kPM * 16 + 16 * w + (l & 15), k = 64 * v + 16 * (l >> 4) + 4 * q + c;
                            wb[((((size_t)w * 8 + v) * 4 + q) * 64 + l) * 4 + c] = u < n ? Wf3[(size_t)u * F + k] : 0.f;
                        }
        P.wfc3b = upload(h, wb, &rc);
        CHECK(rc);
    }
    P.wwide = upload(h, wr, &rc);
    CHECK(rc);
    P.wwide_lds = upload(h, wl, &rc);
    CHECK(rc);
    return WRNN_OK;
}

// Block-sparse wide image of a pruned fatchord RAW model (sparse_wide_pack.h; §3.0g, the wide
// form), built where the wide image exists: per slot the lists of its 13 product sets as
// slot_image lays them out. Weights whose lists do not fit the kernel's LDS carve (50 % density,
// dense weights) get no image and run dense.
int pack_persist_wide_sp(wrnn_handle* h) {
    auto& T = h->host;
    auto& P = h->pw;
    P.wsp_img = nullptr;
    P.wsp_density = 0;
    P.wsp_fill = 0;
    const int H = h->H, F = h->F, A = h->A, n = h->n_classes;
    if (!P.wwide || h->cfg.mode != WRNN_MODE_RAW || (n != kPM * 16 && n != 2 * kPM * 16)) return WRNN_OK;
    const wsp::StepMatrices m{T["rnn2.weight_ih_l0"].data(), T["rnn1.weight_hh_l0"].data(), T["rnn2.weight_hh_l0"].data(),
                              T["fc1.weight"].data(), T["fc2.weight"].data(), T["fc3.weight"].data(),
                              H + A, H, H, H + A, F + A, F, n};
    const wsp::Image im = wsp::build_image(m);
    P.wsp_density = im.density();
    P.wsp_fill = im.fill_f4;
    if (!im.fits) return WRNN_OK;
    std::vector<float> img((size_t)kPM * wsp::kImgWords);  // (the words' bits, moved as bytes)
    for (int w = 0; w < kPM; ++w)
        wsp::slot_image(im.slots[w], reinterpret_cast<uint32_t*>(img.data()) + (size_t)w * wsp::kImgWords);
    int rc = WRNN_OK;
    P.wsp_img = upload(h, img, &rc);
    CHECK(rc);
    return WRNN_OK;
}

// Runtimeracer persistent-engine weight layout (kernels_persist_rr.hip). Slot w, thread tid
// (quad q = tid / 128, og = (tid / 16) % 8, kc = tid % 16, unit u = 8 w + og) holds float4 i:
//   gate block at b: b + 4 j + i = gate j of unit u, k-float4 16 i + kc
//   fc block at b:   b + i       = row u, k-float4 16 i + kc
//   quad 0: W_ih2 @0, W_ih3[:, :256] @12, fc4 @24      quad 1: W_ih4 @0, W_hh1 @12, fc3[:, :256] @24
//   quad 2: W_hh2 @0, W_hh3 @12, fc2 @24               quad 3: W_hh4 @0, fc1[:, :256] @12
// and w5 [slot][32][64 float4]: fc5 row cpw w + c of class c of the slot (LDS-resident).
int pack_persist_rr(wrnn_handle* h, int oG3, int oF1, int oF3) {
    auto& T = h->host;
    const int H = h->H, F = h->F, A = h->A, n = h->n_classes;
    auto& P = h->pw;
    P.ok = false;
    P.rr = true;
    P.gen = false;
    if (h->cfg.model_type != WRNN_MODEL_RUNTIMERACER || H != kRH || F != kRH || n > kPM * 32)
        return WRNN_OK;
    P.cpw = (n + kPM - 1) / kPM;
    P.nw = kRNW;
    std::vector<float> wreg((size_t)kPM * kPT * kRNW * 4, 0.f);
    for (int w = 0; w < kPM; ++w)
        for (int tid = 0; tid < kPT; ++tid) {
            const int q = tid >> 7, og = (tid >> 4) & 7, kc = tid & 15, u = 8 * w + og;
            float* d = wreg.data() + ((size_t)w * kPT + tid) * kRNW * 4;
            auto gate = [&](int b, const char* key, int ld) {
                const auto& W = T[key];
                for (int j = 0; j < 3; ++j)
                    for (int i = 0; i < 4; ++i)
                        std::memcpy(d + 4 * (b + 4 * j + i), &W[(size_t)(j * H + u) * ld + 4 * (16 * i + kc)],
                                    4 * sizeof(float));
            };
            auto fc = [&](int b, const char* key, int ld, int row) {
                const auto& W = T[key];
                for (int i = 0; i < 4; ++i)
                    std::memcpy(d + 4 * (b + i), &W[(size_t)row * ld + 4 * (16 * i + kc)], 4 * sizeof(float));
            };
            switch (q) {
                case 0: gate(0, "rnn2.weight_ih_l0", H); gate(12, "rnn3.weight_ih_l0", H + A); fc(24, "fc4.weight", F, u); break;
                case 1: gate(0, "rnn4.weight_ih_l0", H); gate(12, "rnn1.weight_hh_l0", H); fc(24, "fc3.weight", F + A, u); break;
                case 2: gate(0, "rnn2.weight_hh_l0", H); gate(12, "rnn3.weight_hh_l0", H); fc(24, "fc2.weight", F, u); break;
                default: gate(0, "rnn4.weight_hh_l0", H); fc(12, "fc1.weight", H + A, u); break;
            }
        }
    std::vector<float> w5((size_t)kPM * 32 * kRH, 0.f);
    for (int w = 0; w < kPM; ++w)
        for (int cl = 0; cl < P.cpw; ++cl) {
            const int c = P.cpw * w + cl;
            if (c < n) std::memcpy(&w5[((size_t)w * 32 + cl) * kRH], &T["fc5.weight"][(size_t)c * F], F * sizeof(float));
        }
    int rc = WRNN_OK;
    P.wreg = upload(h, wreg, &rc);
    CHECK(rc);
    P.wlds = upload(h, w5, &rc);
    CHECK(rc);
    CHECK(pack_p1(h, true));
    auto dv = [&](const std::string& key) -> const float* {
        if (!h->dvec.count(key)) h->dvec[key] = upload(h, T[key], &rc);
        return h->dvec[key];
    };
    P.b_ih2 = dv("rnn2.bias_ih_l0");
    P.b_ih4 = dv("rnn4.bias_ih_l0");
    P.b_hh1 = dv("rnn1.bias_hh_l0");
    P.b_hh2 = dv("rnn2.bias_hh_l0");
    P.b_hh3 = dv("rnn3.bias_hh_l0");
    P.b_hh4 = dv("rnn4.bias_hh_l0");
    P.b_f2 = dv("fc2.bias");
    P.b_f4 = dv("fc4.bias");
    P.b_fc3 = dv("fc5.bias");
    CHECK(rc);
    P.oG2 = oG3;
    P.oF1 = oF1;
    P.oF2 = oF3;
    CHECK(pack_persist_wide_rr(h));
    P.ok = true;
    return WRNN_OK;
}

// Runtimeracer wide-row launch weight images (kernels_persist_wide_rr.hip): MFMA A operands.
// Slot w (half A: w < 16, half B: w >= 16; s = w % 16 owns units 16 s .. 16 s + 15 of its half's
// layers), wave v, lane l, tile T, k-step ks: W_T[row 16 s + (l & 15)][input 32 v + 8 (l >> 4) + ks]
// at [w][v][2 T + ks / 4][l] component ks % 4. Tiles of A: W_ih2 r, z, n | W_hh2 r, z, n | W_ih4
// r, z, n | W_hh4 r, z, n | fc2 | fc4; of B: W_hh1 r, z, n | W_ih3[:, :256] r, z, n | W_hh3 r, z,
// n | fc1[:, :256] | fc3[:, :256] | fc5 rows cpw s + 16 j + m (j < n / 256), cpw = n / 16.
// MOL (30 logits): cpw = 16, so fc5 is tile 11 alone, rows 16 s + m < 30 in B slots 0 and 1 and
// zeros in every other slot.
int pack_persist_wide_rr(wrnn_handle* h) {
    auto& T = h->host;
    auto& P = h->pw;
    P.wwide_rr = nullptr;
    const int H = h->H, F = h->F, A = h->A, n = h->n_classes;
    const bool mol = h->cfg.mode == WRNN_MODE_MOL;
    if (H != kRH || F != kRH) return WRNN_OK;
    if (mol ? n != 30 : h->cfg.mode != WRNN_MODE_RAW || (n != 512 && n != 1024)) return WRNN_OK;
    const int cpw = mol ? 16 : n / 16;
    auto g3 = [&](const char* key, int ld, int t, int u, int k) { return T[key][(size_t)(t * H + u) * ld + k]; };
    auto elem = [&](int w, int tile, int m, int k) -> float {
        const int s = w & 15, u = 16 * s + m;
        if (w < 16) {
            switch (tile / 3) {
                case 0: return g3("rnn2.weight_ih_l0", H, tile % 3, u, k);
                case 1: return g3("rnn2.weight_hh_l0", H, tile % 3, u, k);
                case 2: return g3("rnn4.weight_ih_l0", H, tile % 3, u, k);
                case 3: return g3("rnn4.weight_hh_l0", H, tile % 3, u, k);
                default: return tile == 12 ? T["fc2.weight"][(size_t)u * F + k]
                                           : tile == 13 ? T["fc4.weight"][(size_t)u * F + k] : 0.f;
            }
        }
        if (tile < 3) return g3("rnn1.weight_hh_l0", H, tile, u, k);
        if (tile < 6) return g3("rnn3.weight_ih_l0", H + A, tile - 3, u, k);
        if (tile < 9) return g3("rnn3.weight_hh_l0", H, tile - 6, u, k);
        if (tile == 9) return T["fc1.weight"][(size_t)u * (H + A) + k];
        if (tile == 10) return T["fc3.weight"][(size_t)u * (F + A) + k];
        const int c = cpw * s + 16 * (tile - 11) + m;
        return tile - 11 < cpw / 16 && c < n ? T["fc5.weight"][(size_t)c * F + k] : 0.f;
    };
    std::vector<float> wr(persist_wide_rr_wreg_floats(), 0.f);
    const int nq = (int)(wr.size() / ((size_t)kPM * 8 * 64 * 4));  // float4 per lane (30)
    for (int w = 0; w < kPM; ++w)
        for (int v = 0; v < 8; ++v)
            for (int l = 0; l < 64; ++l)
                for (int q = 0; q < nq; ++q)
                    for (int c = 0; c < 4; ++c) {
                        const int tile = q / 2, ks = 4 * (q % 2) + c;
                        wr[((((size_t)w * 8 + v) * nq + q) * 64 + l) * 4 + c] =
                            elem(w, tile, l & 15, 32 * v + 8 * (l >> 4) + ks);
                    }
    int rc = WRNN_OK;
    P.wwide_rr = upload(h, wr, &rc);
    CHECK(rc);
    return WRNN_OK;
}

// Geneing persistent-engine weight layout (kernels_persist_gen.hip). Slot w, thread tid
// (quad q = tid / 128, og = (tid / 16) % 8, kc = tid % 16) holds float4 i:
//   quad 0: W_hh1 gate j of unit 8 w + og, k-float4 16 i + kc @ 4 j + i (i < 4)
//   quad 1: fc1[:, :256] row 4 w + og (og < 4), k-float4 16 i + kc @ i (i < 4)
//   every quad: fc3 row of class cpw w + 8 q + og, k-float4 16 i + kc @ 12 + i (i < 2)
int pack_persist_gen(wrnn_handle* h, int oF1) {
    auto& T = h->host;
    const int H = h->H, F = h->F, A = h->A, n = h->n_classes;
    auto& P = h->pw;
    P.ok = false;
    P.rr = false;
    P.gen = true;
    if (h->cfg.model_type != WRNN_MODEL_GENEING || H != kRH || F != kGF || n > kPM * 32) return WRNN_OK;
    P.cpw = (n + kPM - 1) / kPM;
    P.nw = kGNW;
    std::vector<float> wreg((size_t)kPM * kPT * kGNW * 4, 0.f);
    const auto& Whh = T["rnn1.weight_hh_l0"];
    const auto& Wf1 = T["fc1.weight"];
    const auto& Wf3 = T["fc3.weight"];
    for (int w = 0; w < kPM; ++w)
        for (int tid = 0; tid < kPT; ++tid) {
            const int q = tid >> 7, og = (tid >> 4) & 7, kc = tid & 15;
            float* d = wreg.data() + ((size_t)w * kPT + tid) * kGNW * 4;
            if (q == 0)
                for (int j = 0; j < 3; ++j)
                    for (int i = 0; i < 4; ++i)
                        std::memcpy(d + 4 * (4 * j + i), &Whh[(size_t)(j * H + 8 * w + og) * H + 4 * (16 * i + kc)],
                                    4 * sizeof(float));
            if (q == 1 && og < F / kPM)
                for (int i = 0; i < 4; ++i)
                    std::memcpy(d + 4 * i, &Wf1[(size_t)(F / kPM * w + og) * (H + A) + 4 * (16 * i + kc)],
                                4 * sizeof(float));
            const int cl = 8 * q + og, c = P.cpw * w + cl;
            if (cl < P.cpw && c < n)
                for (int i = 0; i < 2; ++i)
                    std::memcpy(d + 4 * (12 + i), &Wf3[(size_t)c * F + 4 * (16 * i + kc)], 4 * sizeof(float));
        }
    int rc = WRNN_OK;
    P.wreg = upload(h, wreg, &rc);
    CHECK(rc);
    P.wlds = nullptr;
    CHECK(pack_p1(h, true));
    auto dv = [&](const std::string& key) -> const float* {
        if (!h->dvec.count(key)) h->dvec[key] = upload(h, T[key], &rc);
        return h->dvec[key];
    };
    P.b_hh1 = dv("rnn1.bias_hh_l0");
    P.b_fc3 = dv("fc3.bias");
    CHECK(rc);
    P.oF1 = oF1;
    CHECK(pack_persist_wide_gen(h));
    P.ok = true;
    return WRNN_OK;
}

// Geneing wide-row launch weight image (kernels_persist_wide_gen.hip): MFMA A operands. Slot w,
// wave v, lane l (tile row m = l & 15, k-group c = l >> 4). K = 256 tiles T = 0..2, k-step ks < 8:
// W_T[m][input 32 v + 8 c + ks] at [w][v][2 T + ks / 4][l] component ks % 4, with T0 = W_hh1 gate r
// of unit 8 w + m (m < 8) | gate z of unit 8 w + m - 8, T1 = gate n of unit 8 w + m (m < 8) | 0,
// T2 = fc1[:, :256] row 4 w + m (m < 4) | 0. fc3 tiles j = 0, 1 (K = 128), k-step ks < 4: fc3 row
// cpw w + 16 j + m, input 16 v + 4 c + ks at [w][v][6 + j][l] component ks; cpw = n / 32.
// MOL (n = 30) / BETA (n = 2): cpw = 16, one fc3 tile, rows >= n zero (slots 2-31 hold a zero image).
int pack_persist_wide_gen(wrnn_handle* h) {
    auto& T = h->host;
    auto& P = h->pw;
    P.wwide_gen = nullptr;
    const int H = h->H, F = h->F, A = h->A, n = h->n_classes;
    const int mode = h->cfg.mode;
    const bool bits = mode == WRNN_MODE_RAW && (n == 512 || n == 1024);
    const bool cont = (mode == WRNN_MODE_MOL && n == 30) || (mode == WRNN_MODE_BETA && n == 2);
    if (H != kRH || F != kGF || !(bits || cont)) return WRNN_OK;
    const int cpw = bits ? n / kPM : 16;
    const auto& Whh = T["rnn1.weight_hh_l0"];
    const auto& Wf1 = T["fc1.weight"];
    const auto& Wf3 = T["fc3.weight"];
    std::vector<float> wr(persist_wide_gen_wreg_floats(), 0.f);
    const int nq = (int)(wr.size() / ((size_t)kPM * 8 * 64 * 4));  // float4 per lane (8)
    for (int w = 0; w < kPM; ++w)
        for (int v = 0; v < 8; ++v)
            for (int l = 0; l < 64; ++l) {
                const int m = l & 15, c = l >> 4;
                float* d = wr.data() + (((size_t)w * 8 + v) * nq * 64 + l) * 4;  // + q * 256
                for (int ks = 0; ks < 8; ++ks) {
                    const int k = 32 * v + 8 * c + ks;
                    const size_t at = (size_t)(ks / 4) * 256 + ks % 4;
                    d[0 * 256 + at] = Whh[(size_t)((m < 8 ? 0 : 1) * H + 8 * w + (m & 7)) * H + k];
                    if (m < 8) d[2 * 256 + at] = Whh[(size_t)(2 * H + 8 * w + m) * H + k];
                    if (m < F / kPM) d[4 * 256 + at] = Wf1[(size_t)(F / kPM * w + m) * (H + A) + k];
                }
                for (int j = 0; j < cpw / 16; ++j)
                    for (int ks = 0; ks < 4; ++ks)
                        if (cpw * w + 16 * j + m < n)
                            d[(6 + j) * 256 + ks] = Wf3[(size_t)(cpw * w + 16 * j + m) * F + 16 * v + 4 * c + ks];
            }
    int rc = WRNN_OK;
    P.wwide_gen = upload(h, wr, &rc);
    CHECK(rc);
    return WRNN_OK;
}

int do_finalize(wrnn_handle* h) {
    if (const char* env = std::getenv("WRNN_NRG")) {
        const int v = std::atoi(env);
        if (v != 1 && v != 2 && v != 4) return fail(WRNN_ERR_INVALID, "WRNN_NRG must be 1, 2 or 4");
        h->nrg = v;
    }
    for (auto& kv : h->expected)
        if (!h->host.count(kv.first))
            return fail(WRNN_ERR_INVALID, "missing state-dict tensor '" + kv.first + "'");
    auto& T = h->host;
    int rc = WRNN_OK;
    const int C = h->C, H = h->H, F = h->F, A = h->A, n = h->n_classes;
    h->wbufs.clear();
    h->stages.clear();
    h->auxc.clear();
    h->dvec.clear();
    h->Wres.clear();
    h->upk.clear();
    // ---- upsample network
    h->Wci = upload(h, T["upsample.resnet.conv_in.weight"], &rc);
    CHECK(rc);
    std::vector<float> alpha, beta;
    auto push_bn = [&](const std::string& p) {
        const auto& w = T[p + ".weight"];
        const auto& b = T[p + ".bias"];
        const auto& m = T[p + ".running_mean"];
        const auto& v = T[p + ".running_var"];
        for (int c = 0; c < C; ++c) {
            // torch CPU eval batch_norm: invstd = 1/sqrt(var+eps); alpha = invstd*w;
            // beta = b - mean*alpha (aten/native/cpu/batch_norm_kernel.cpp)
            volatile float vs = v[c] + 1e-5f;
            volatile float sq = std::sqrt((float)vs);
            volatile float invstd = 1.0f / (float)sq;
            volatile float al = (float)invstd * w[c];
            volatile float mb = m[c] * (float)al;
            alpha.push_back((float)al);
            beta.push_back(b[c] - (float)mb);
        }
    };
    push_bn("upsample.resnet.batch_norm");
    for (int i = 0; i < h->cfg.res_blocks; ++i) {
        const std::string p = "upsample.resnet.layers." + std::to_string(i);
        push_bn(p + ".batch_norm1");
        push_bn(p + ".batch_norm2");
        h->Wres.push_back(upload(h, T[p + ".conv1.weight"], &rc));
        CHECK(rc);
        h->Wres.push_back(upload(h, T[p + ".conv2.weight"], &rc));
        CHECK(rc);
    }
    h->bn_a = upload(h, alpha, &rc);
    CHECK(rc);
    h->bn_b = upload(h, beta, &rc);
    CHECK(rc);
    h->Wco = upload(h, T["upsample.resnet.conv_out.weight"], &rc);
    CHECK(rc);
    h->bco = upload(h, T["upsample.resnet.conv_out.bias"], &rc);
    CHECK(rc);
    for (int j = 0; j < h->cfg.n_upsample; ++j) {
        h->upk.push_back(upload(h, T["upsample.up_layers." + std::to_string(2 * j + 1) + ".weight"], &rc));
        CHECK(rc);
    }
    // ---- input layer I: x0 = [x, mel(80), a1[:A-1]] (fatchord_version.py:198-199)
    const auto& WI = T["I.weight"];
    const int ldI = h->feat + A;
    h->KI = h->feat + A - 1;
    h->WIT = upload(h, transpose_cols(WI, H, ldI, 1, h->KI), &rc);
    CHECK(rc);
    h->bI = upload(h, T["I.bias"], &rc);
    CHECK(rc);
    std::vector<float> w0(H);
    for (int o = 0; o < H; ++o) w0[o] = WI[(size_t)o * ldI];
    h->w0 = upload(h, w0, &rc);
    CHECK(rc);
    // v = W_ih1 . w0 (the rank-1 x-term of rnn1's input projection)
    {
        const auto& Wih1 = T["rnn1.weight_ih_l0"];
        std::vector<float> v(3 * H);
        for (int o = 0; o < 3 * H; ++o) {
            double s = 0;
            for (int k = 0; k < H; ++k) s += (double)Wih1[(size_t)o * H + k] * (double)w0[k];
            v[o] = (float)s;
        }
        h->v1 = upload(h, v, &rc);
        CHECK(rc);
    }
    auto dv = [&](const std::string& key) -> const float* {
        if (!h->dvec.count(key)) {
            h->dvec[key] = upload(h, T[key], &rc);
        }
        return h->dvec[key];
    };
    // ---- aux conditioning (per frame): W_aux^T (A, n_out) + bias
    int off = 0;
    auto add_aux = [&](int slice, const std::string& wname, const std::string& bname, int rows,
                       int ld, int col0) {
        wrnn_handle::AuxCond ac;
        ac.slice = slice;
        ac.n_out = rows;
        ac.offset = off;
        ac.WT = upload(h, transpose_cols(T[wname], rows, ld, col0, A), &rc);
        ac.bias = dv(bname);
        off += rows;
        h->auxc.push_back(ac);
        return ac.offset;
    };
    const int K = H;  // recurrent inner dimension
    const bool geneing = h->cfg.model_type == WRNN_MODEL_GENEING;
    if (!geneing && H != F) return fail(WRNN_ERR_INVALID, "rnn_dims != fc_dims is not supported");
    if (K != 256 && K != 512)
        return fail(WRNN_ERR_INVALID, "rnn_dims must be 256 or 512 (got " + std::to_string(K) + ")");
    if (geneing && F != 128 && F != 256 && F != 512)
        return fail(WRNN_ERR_INVALID, "fc_dims must be 128, 256 or 512 (got " + std::to_string(F) + ")");
    if (F < 256 && h->nrg < 2) h->nrg = 2;  // K = 128 tiles need >= 4 k per thread
    if (h->cfg.mode == WRNN_MODE_RAW && n % 4)
        return fail(WRNN_ERR_INVALID, "n_classes must be a multiple of 4");
    auto seg_gru = [&](const std::string& gname, int col0_ld, int x, int gh, int hh, int xout,
                       const float* cond, int fc) {
        SegDesc s{};
        s.w = pack_segment(h, T[gname + ".weight_ih_l0"], 3 * H, col0_ld, 0, K, TILE_GATE, H, &rc);
        s.kind = EPI_GRU;
        s.x = x;
        s.y = SL_NONE;
        s.cond = cond;
        s.c_ld = fc >= 0 ? -1 : 0;
        s.fcol = fc;
        s.gh = gh;
        s.h = hh;
        s.xout = xout;
        return s;
    };
    auto seg_hh = [&](const std::string& gname, int hsl, int ghsl) {
        SegDesc s{};
        s.w = pack_segment(h, T[gname + ".weight_hh_l0"], 3 * H, H, 0, K, TILE_GATE, H, &rc);
        s.kind = EPI_BIAS3;
        s.x = hsl;
        s.y = ghsl;
        s.cond = dv(gname + ".bias_hh_l0");
        s.c_ld = 0;
        s.fcol = -1;
        s.gh = s.h = s.xout = SL_NONE;
        return s;
    };
    auto seg_p1 = [&]() {
        SegDesc s{};
        s.w = pack_segment(h, T["rnn1.weight_ih_l0"], 3 * H, H, 0, K, TILE_GATE, H, &rc);
        s.kind = EPI_BIAS3;
        s.x = SL_CI;
        s.y = SL_P1;
        s.cond = dv("rnn1.bias_ih_l0");
        s.c_ld = 0;
        s.fcol = -1;
        s.gh = s.h = s.xout = SL_NONE;
        return s;
    };
    auto seg_fc = [&](const std::string& nm, int n_out, int ld, int x, int y, bool relu,
                      const float* cond, int fc, int Kin = 0) {
        SegDesc s{};
        s.w = pack_segment(h, T[nm + ".weight"], n_out, ld, 0, Kin ? Kin : K, TILE_OUT, 0, &rc);
        s.kind = relu ? EPI_COND_RELU : EPI_COND;
        s.x = x;
        s.y = y;
        s.cond = cond;
        s.c_ld = fc >= 0 ? -1 : 0;
        s.fcol = fc;
        s.gh = s.h = s.xout = SL_NONE;
        return s;
    };
    auto fcol = [](int offset) { return offset; };
    if (h->cfg.model_type == WRNN_MODEL_FATCHORD) {
        const int oG2 = add_aux(1, "rnn2.weight_ih_l0", "rnn2.bias_ih_l0", 3 * H, H + A, H);
        const int oF1 = add_aux(2, "fc1.weight", "fc1.bias", F, H + A, H);
        const int oF2 = add_aux(3, "fc2.weight", "fc2.bias", F, F + A, F);
        CHECK(rc);
        h->cond_width = off;
        StageDesc s0{"gru2", K, {}, false};
        s0.segs.push_back(seg_gru("rnn2", H + A, SL_X1, SL_GH2, SL_H2, SL_X2, nullptr, fcol(oG2)));
        s0.segs.push_back(seg_hh("rnn1", SL_H1, SL_GH1));
        StageDesc s1{"fc1", K, {}, false};
        s1.segs.push_back(seg_fc("fc1", F, H + A, SL_X2, SL_Y1, true, nullptr, fcol(oF1)));
        s1.segs.push_back(seg_hh("rnn2", SL_H2, SL_GH2));
        StageDesc s2{"fc2", K, {}, true};
        s2.segs.push_back(seg_fc("fc2", F, F + A, SL_Y1, SL_Y2, true, nullptr, fcol(oF2)));
        s2.segs.push_back(seg_p1());
        StageDesc s3{"fc3", K, {}, false};
        s3.segs.push_back(seg_fc("fc3", n, F, SL_Y2, SL_LOG, false, dv("fc3.bias"), -1));
        CHECK(rc);
        h->stages = {s0, s1, s2, s3};
        CHECK(pack_persist(h, oG2, oF1, oF2));
    } else if (geneing) {
        // geneing_version.py:193-205: x1 = I(x0) + rnn1(...) ; y1 = relu(fc1([x1, a2])) ;
        // logits = fc3(y1). Stage 0 (K = H): fc1, W_hh1 h1, P1 of the next step; stage 1
        // (K = F): fc3. GRU1 runs in the sampler.
        h->pw.ok = false;
        h->pw.rr = false;
        const int oF1 = add_aux(1, "fc1.weight", "fc1.bias", F, H + A, H);
        CHECK(rc);
        h->cond_width = off;
        StageDesc s0{"fc1", K, {}, true};
        s0.segs.push_back(seg_fc("fc1", F, H + A, SL_X1, SL_Y1, true, nullptr, fcol(oF1)));
        s0.segs.push_back(seg_hh("rnn1", SL_H1, SL_GH1));
        s0.segs.push_back(seg_p1());
        StageDesc s1{"fc3", F, {}, false};
        s1.segs.push_back(seg_fc("fc3", n, F, SL_Y1, SL_LOG, false, dv("fc3.bias"), -1, F));
        CHECK(rc);
        h->stages = {s0, s1};
        CHECK(pack_persist_gen(h, oF1));
    } else {
        h->pw.ok = false;
        h->pw.rr = false;
        const int oG3 = add_aux(1, "rnn3.weight_ih_l0", "rnn3.bias_ih_l0", 3 * H, H + A, H);
        const int oF1 = add_aux(2, "fc1.weight", "fc1.bias", F, H + A, H);
        const int oF3 = add_aux(3, "fc3.weight", "fc3.bias", F, F + A, F);
        CHECK(rc);
        h->cond_width = off;
        StageDesc s0{"gru2", K, {}, false};
        s0.segs.push_back(seg_gru("rnn2", H, SL_X1, SL_GH2, SL_H2, SL_X2, dv("rnn2.bias_ih_l0"), -1));
        s0.segs.push_back(seg_hh("rnn1", SL_H1, SL_GH1));
        StageDesc s1{"gru3", K, {}, false};
        s1.segs.push_back(seg_gru("rnn3", H + A, SL_X2, SL_GH3, SL_H3, SL_X3, nullptr, fcol(oG3)));
        s1.segs.push_back(seg_hh("rnn2", SL_H2, SL_GH2));
        StageDesc s2{"gru4", K, {}, false};
        s2.segs.push_back(seg_gru("rnn4", H, SL_X3, SL_GH4, SL_H4, SL_X4, dv("rnn4.bias_ih_l0"), -1));
        s2.segs.push_back(seg_hh("rnn3", SL_H3, SL_GH3));
        StageDesc s3{"fc1", K, {}, false};
        s3.segs.push_back(seg_fc("fc1", F, H + A, SL_X4, SL_Y1, false, nullptr, fcol(oF1)));
        s3.segs.push_back(seg_hh("rnn4", SL_H4, SL_GH4));
        StageDesc s4{"fc2", K, {}, true};
        s4.segs.push_back(seg_fc("fc2", F, F, SL_Y1, SL_Y2, true, dv("fc2.bias"), -1));
        s4.segs.push_back(seg_p1());
        StageDesc s5{"fc3", K, {}, false};
        s5.segs.push_back(seg_fc("fc3", F, F + A, SL_Y2, SL_Y3, false, nullptr, fcol(oF3)));
        StageDesc s6{"fc4", K, {}, false};
        s6.segs.push_back(seg_fc("fc4", F, F, SL_Y3, SL_Y4, true, dv("fc4.bias"), -1));
        StageDesc s7{"fc5", K, {}, false};
        s7.segs.push_back(seg_fc("fc5", n, F, SL_Y4, SL_LOG, false, dv("fc5.bias"), -1));
        CHECK(rc);
        h->stages = {s0, s1, s2, s3, s4, s5, s6, s7};
        CHECK(pack_persist_rr(h, oG3, oF1, oF3));
    }
    CHECK(rc);
    // per-frame cond pointers: mark with c_ld = -1 -> resolved against ws.fcond at launch
    h->finalized = true;
    for (auto& kv : h->graphs) (void)hipGraphExecDestroy(kv.second);
    h->graphs.clear();
    return WRNN_OK;
}

int pick_rt(int B, int* nrt) {
    static const int opts[] = {4, 8, 12, 16, 20, 24, 32};
    if (B <= 32) {
        for (int o : opts)
            if (o >= B) {
                *nrt = 1;
                return o;
            }
    }
    int best = 32, bw = 1 << 30;
    for (int o : {16, 20, 24, 32}) {
        const int t = (B + o - 1) / o;
        const int w = t * o - B;
        if (w < bw || (w == bw && o > best)) {
            bw = w;
            best = o;
        }
    }
    *nrt = (B + best - 1) / best;
    return best;
}

int ensure_workspace(wrnn_handle* h, int B, int S, int Pneed, int Fneed, int Tmax, int Tsum) {
    auto& ws = h->ws;
    const bool grow = B > ws.B || S > ws.S || Pneed > ws.Pcap || Fneed > ws.Fcap || Tmax > ws.Tcap ||
                      Tsum > ws.Ncap;
    if (!grow) return WRNN_OK;
    for (auto& kv : h->graphs) (void)hipGraphExecDestroy(kv.second);
    h->graphs.clear();
    const int nB = std::max(B, ws.B), nS = std::max(S, ws.S);
    const int nP = std::max(Pneed, ws.Pcap), nF = std::max(Fneed, ws.Fcap), nT = std::max(Tmax, ws.Tcap);
    const int nN = std::max(Tsum, ws.Ncap);
    for (int s = 0; s < SL_CI; ++s) {
        const int w = h->slot_width(s);
        if (w == 0) continue;
        ws.slots[s].release();
        CHECK(ws.slots[s].alloc((size_t)nB * w * sizeof(float)));
    }
    ws.labels.release();
    ws.samples.release();
    ws.noise.release();
    ws.cI.release();
    ws.fcond.release();
    ws.rows.release();
    CHECK(ws.labels.alloc((size_t)nB * nS * sizeof(int16_t)));
    CHECK(ws.samples.alloc((size_t)nB * nS * sizeof(float)));
    CHECK(ws.cI.alloc((size_t)nS * nB * h->H * sizeof(float)));  // folded [t][row][H]
    CHECK(ws.fcond.alloc((size_t)nF * h->cond_width * sizeof(float)));
    CHECK(ws.rows.alloc((size_t)nB * sizeof(RowInfo)));
    // MelResNet activations of every utterance of a call side by side (nN frame columns);
    // mel upsample scratch for one utterance of <= nT frames
    const int tot = h->hop;  // product of factors
    ws.act0.release();
    ws.act1.release();
    ws.Rb.release();
    ws.up1.release();
    ws.up2.release();
    ws.melup.release();
    CHECK(ws.act0.alloc((size_t)h->C * nN * sizeof(float)));
    CHECK(ws.act1.alloc((size_t)h->C * nN * sizeof(float)));
    CHECK(ws.Rb.alloc((size_t)h->R * nN * sizeof(float)));
    size_t w1 = (size_t)(nT + 2 * h->cfg.pad) * h->cfg.upsample_factors[0];
    size_t w2 = w1 * (h->cfg.n_upsample > 1 ? h->cfg.upsample_factors[1] : 1);
    CHECK(ws.up1.alloc((size_t)h->feat * w1 * sizeof(float)));
    CHECK(ws.up2.alloc((size_t)h->feat * w2 * sizeof(float)));
    CHECK(ws.melup.alloc((size_t)h->feat * nT * tot * sizeof(float)));
    ws.B = nB;
    ws.S = nS;
    ws.Pcap = nP;
    ws.Fcap = nF;
    ws.Tcap = nT;
    ws.Ncap = nN;
    return WRNN_OK;
}

// Per-frame P1 (pack_p1) unless WRNN_P1_FRAMES=0 (A/B against the per-(step, row) GEMM).
static bool p1_frames_enabled() {
    static const bool on = [] {
        const char* env = std::getenv("WRNN_P1_FRAMES");
        return !(env && std::atoi(env) == 0);
    }();
    return on;
}

// The fatchord register-resident kernel can form P1 in-kernel (per-frame form available).
// WRNN_P1_RING=0 (read per call) keeps the stream for every kernel (A/B, tests: the ring and
// the stream carry bit-identical values).
static bool p1_ring_ok(const wrnn_handle* h) {
    const char* env = std::getenv("WRNN_P1_RING");
    if (env && std::atoi(env) == 0) return false;
    return !h->pw.rr && !h->pw.gen && h->pw.p1x4 && h->pw.p1taps_ok && h->pw.p1split >= 0 &&
           p1_frames_enabled();
}

// The runtimeracer wide kernel forms P1 from the per-frame projections (its A half, for the
// partner B slot) when the 4-tap form exists; else it reads the [S][B][4H] stream.
static bool rr_frames_ok(const wrnn_handle* h) {
    const char* env = std::getenv("WRNN_P1_RING");
    if (env && std::atoi(env) == 0) return false;
    return h->pw.rr && h->pw.p1x4 && h->pw.p1taps_ok && h->pw.p1split >= 0 && p1_frames_enabled();
}

// ---- MelResNet of every utterance of a call as one batch of frame columns ---------------
// fatchord_version.py:27-44 (runtimeracer / geneing the same): conv_in (k = 2 pad + 1, no
// padding) per utterance -- its im2col reads that utterance's zero-padded mel -- into its own
// columns [col0, col0 + T) of act0, then the 2 x res_blocks 1x1 convs (BatchNorm folded, ReLU /
// residual) and conv_out over all N = sum(T) columns at once: one launch per layer for the
// whole call instead of one per layer and utterance.
int run_resnet(wrnn_handle* h, int n_utts, const float* const* mels, const int* T, const int* col0, int N) {
    auto& ws = h->ws;
    hipStream_t st = h->stream;
    const int C = h->C, R = h->R;
    const int ksz = 2 * h->cfg.pad + 1;
    if (N > ws.Ncap) return fail(WRNN_ERR_INVALID, "MelResNet columns exceed the workspace");
    ws.N = N;
    for (int u = 0; u < n_utts; ++u) {
        GemmA a{};
        GemmB b{};
        GemmEp e{};
        a.kind = 0;
        a.p = h->Wci;
        a.ld = h->feat * ksz;
        b.kind = 1;  // im2col: out frame n uses padded[n + kk] = mel[n + kk - pad]
        b.p = mels[u];
        b.T = T[u];
        b.pad = h->cfg.pad;
        b.ksz = ksz;
        e.kind = 2;
        e.D = ws.act0.f() + col0[u];
        e.ld = N;
        e.alpha = h->bn_a;
        e.beta = h->bn_b;
        e.relu = 1;
        e.res = nullptr;
        HIPC(launch_gemm(C, T[u], h->feat * ksz, a, b, e, st));
    }
    for (int i = 0; i < h->cfg.res_blocks; ++i) {
        GemmA a1{};
        GemmB b1{};
        GemmEp e1{};
        a1.kind = 0;
        a1.p = h->Wres[2 * i];
        a1.ld = C;
        b1.kind = 0;
        b1.p = ws.act0.f();
        b1.ld = N;
        e1.kind = 2;
        e1.D = ws.act1.f();
        e1.ld = N;
        e1.alpha = h->bn_a + (size_t)(1 + 2 * i) * C;
        e1.beta = h->bn_b + (size_t)(1 + 2 * i) * C;
        e1.relu = 1;
        HIPC(launch_gemm(C, N, C, a1, b1, e1, st));
        GemmA a2{};
        GemmB b2{};
        GemmEp e2{};
        a2.kind = 0;
        a2.p = h->Wres[2 * i + 1];
        a2.ld = C;
        b2.kind = 0;
        b2.p = ws.act1.f();
        b2.ld = N;
        e2.kind = 2;
        e2.D = ws.act0.f();
        e2.ld = N;
        e2.alpha = h->bn_a + (size_t)(2 + 2 * i) * C;
        e2.beta = h->bn_b + (size_t)(2 + 2 * i) * C;
        e2.relu = 0;
        e2.res = ws.act0.f();
        HIPC(launch_gemm(C, N, C, a2, b2, e2, st));
    }
    GemmA a3{};
    GemmB b3{};
    GemmEp e3{};
    a3.kind = 0;
    a3.p = h->Wco;
    a3.ld = C;
    b3.kind = 0;
    b3.p = ws.act0.f();
    b3.ld = N;
    e3.kind = 1;
    e3.D = ws.Rb.f();
    e3.ld = N;
    e3.bias = h->bco;
    HIPC(launch_gemm(R, N, C, a3, b3, e3, st));
    return WRNN_OK;
}

// ---- upsample + conditioning for one utterance (its MelResNet output: Rb columns col0..) --
int run_upsample(wrnn_handle* h, const float* d_mel, int T, int Bu, int tpo, int S, int Btot,
                 int row0, int fbase, float* P1out, int col0, int f0) {
    auto& ws = h->ws;
    hipStream_t st = h->stream;
    const int H = h->H;
    const int L = T * h->hop;
    const float* Rb = ws.Rb.f() + col0;  // aux channel c of frame f: Rb[c * ws.N + f]
    // PERSIST with the per-frame P1 (pack_p1): no upsampled mel is needed at all
    const bool p1f = P1out && h->pw.p1x4 && h->pw.p1taps_ok && p1_frames_enabled();
    h->melup_valid = !p1f;
    // mel stretch+conv stencils (fatchord_version.py:68-76,83-84)
    if (!p1f) {
        const int nu = h->cfg.n_upsample;
        const float* src = d_mel;
        int in_pad = h->cfg.pad, T_in = T, W_in = T + 2 * h->cfg.pad;
        float* bufs[2] = {ws.up1.f(), ws.up2.f()};
        for (int j = 0; j < nu; ++j) {
            const int s = h->cfg.upsample_factors[j];
            const int W_out = W_in * s;
            const bool last = j == nu - 1;
            float* dst = last ? ws.melup.f() : bufs[j & 1];
            const int lo = last ? h->indent : 0;
            const int len = last ? W_out - 2 * h->indent : W_out;
            if (last && len != L) return fail(WRNN_ERR_INVALID, "upsample length mismatch");
            HIPC(launch_mel_stencil(src, in_pad, T_in, W_in, dst, s, h->upk[j], h->feat, lo, len,
                                    len, st));
            src = dst;
            in_pad = 0;
            T_in = W_out;
            W_in = W_out;
        }
    }
    // cI(t, row) = I.weight[:,1:] . [mel_up(p), aux(p)[:A-1]] + I.bias, p = fold*tpo + t,
    // written in the folded step-major layout [t][row][H] the recurrence reads contiguously
    {
        GemmA a4{};
        GemmB b4{};
        GemmEp e4{};
        a4.kind = 1;
        a4.mel = ws.melup.f();
        a4.ldm = L;
        a4.n_mel = h->feat;
        a4.L = L;
        a4.hop = h->hop;
        a4.R = Rb;
        a4.ldr = ws.N;
        a4.r_off = 0;
        a4.n_aux = h->A - 1;
        a4.Bu = Bu;
        a4.tpo = tpo;
        a4.f0 = f0;
        b4.kind = 0;
        b4.p = h->WIT;
        b4.ld = H;
        e4.kind = 3;
        e4.D = ws.cI.f();
        e4.ld = H;
        e4.bias = h->bI;
        e4.Bu = Bu;
        e4.Btot = Btot;
        e4.row0 = row0;
        // the x4 P1 carries cI as its fourth column: the persistent kernels never read ws.cI
        if (!(P1out && h->pw.p1x4)) HIPC(launch_gemm(S * Bu, H, h->KI, a4, b4, e4, st));
        if (p1f) {  // PERSIST, per-frame form: Q = M1_mel mel, Aq = M1_aux aux + bP1, then taps
            const int np = 4 * H;  // frame slots [fbase, fbase + T] of this utterance
            if ((size_t)(fbase + T + 3) * np * sizeof(float) > ws.q4.bytes || fbase < 1)
                return fail(WRNN_ERR_INVALID, "frame slots exceed the workspace");
            GemmA aq{};
            GemmB bq{};
            GemmEp eq{};
            aq.kind = 2;  // frame-A: slot 0 = zero frame, slot j + 1 = frame j
            aq.R = d_mel;
            aq.ldr = T;
            aq.r_off = 0;
            bq.kind = 0;
            bq.p = h->pw.M1T;
            bq.ld = np;
            eq.kind = 0;
            eq.D = ws.q4.f() + (size_t)fbase * np;
            eq.ld = np;
            eq.bias = h->pw.zero_np;
            HIPC(launch_gemm(T + 1, np, h->feat, aq, bq, eq, st));
            aq.R = Rb;  // aux channels 0 .. A-2 (the I slice, as a4.r_off / n_aux)
            aq.ldr = ws.N;
            bq.p = h->pw.M1T + (size_t)h->feat * np;
            eq.D = ws.a4.f() + (size_t)fbase * np;
            eq.bias = h->pw.bP1;
            HIPC(launch_gemm(T + 1, np, h->A - 1, aq, bq, eq, st));
            // the whole stream for the kernels that read it; step 0 only when every launch
            // forms P1 in-kernel (k_persist_init reads step 0)
            HIPC(launch_p1_expand(P1out, Btot, row0, Bu, f0, h->p1_stream ? S : 1, tpo, L, h->hop, T,
                                  np / 4, ws.q4.f() + (size_t)fbase * np,
                                  ws.a4.f() + (size_t)fbase * np, h->pw.p1taps, st));
        } else if (P1out) {  // PERSIST: P1 (step, row) = M1 c + bP1, same gather, same folded layout
            const int np = h->pw.p1x4 ? 4 * H : 3 * H;  // (fatchord: + cI, unit-major)
            b4.p = h->pw.M1T;
            b4.ld = np;
            e4.D = P1out;
            e4.ld = np;
            e4.bias = h->pw.bP1;
            HIPC(launch_gemm(S * Bu, np, h->KI, a4, b4, e4, st));
        }
    }
    // per-frame aux conditioning, slot 0 = zero frame
    for (const auto& ac : h->auxc) {
        GemmA a5{};
        GemmB b5{};
        GemmEp e5{};
        a5.kind = 2;
        a5.R = Rb;
        a5.ldr = ws.N;
        a5.r_off = ac.slice * h->A;
        b5.kind = 0;
        b5.p = ac.WT;
        b5.ld = ac.n_out;
        e5.kind = 0;
        e5.D = ws.fcond.f() + (size_t)fbase * h->cond_width + ac.offset;
        e5.ld = h->cond_width;
        e5.bias = ac.bias;
        HIPC(launch_gemm(T + 1, ac.n_out, h->A, a5, b5, e5, st));
    }
    return WRNN_OK;
}

// Build the StageArgs of stage `si` at step t.
int build_stage_args(wrnn_handle* h, int si, int t, int S, bool timing, StageArgs* out, int* K) {
    const StageDesc& sd = h->stages[si];
    auto& ws = h->ws;
    StageArgs a{};
    a.nrows = h->last_B;
    a.t = t;
    a.hop = h->hop;
    a.rows = (const RowInfo*)ws.rows.p;
    a.stamps = nullptr;
    if (timing && t >= 0 && t % kStampEvery == 0)
        a.stamps = (uint32_t*)ws.stamps.p +
                   ((size_t)(t / kStampEvery) * h->stages.size() + si) * kMaxStampWG * 2;
    a.phases = nullptr;
    if (t >= 0 && t == h->phase_step && h->phases.p)
        a.phases = (uint32_t*)h->phases.p + (size_t)si * kMaxStampWG * 8;
    int ns = 0, tile = 0;
    for (size_t k = 0; k < sd.segs.size(); ++k) {
        const SegDesc& d = sd.segs[k];
        if (d.x == SL_CI && t + 1 >= S) continue;  // no next step
        Seg& g = a.seg[ns];
        g.W = d.w.W->f();
        g.n_out = d.w.n_out;
        g.n_tiles = d.w.n_tiles;
        g.kind = d.kind;
        g.cfg = d.w.cfg;
        g.H = h->H;
        if (d.x == SL_CI) {
            g.X = ws.cI.f();
            g.x_off = (long long)(t + 1) * h->last_B * h->H;
            g.x_ld = h->H;
            g.x_pld = 0;
        } else {
            g.X = h->slot(d.x);
            g.x_off = 0;
            g.x_ld = h->slot_width(d.x);
            g.x_pld = 0;
        }
        g.Y = d.y >= 0 ? h->slot(d.y) : nullptr;
        g.y_ld = d.y >= 0 ? h->slot_width(d.y) : 0;
        if (d.c_ld < 0) {  // per-frame conditioning column offset
            g.cond = ws.fcond.f() + d.fcol;
            g.c_ld = h->cond_width;
        } else {
            g.cond = d.cond;
            g.c_ld = 0;
        }
        g.gh = d.gh >= 0 ? h->slot(d.gh) : nullptr;
        g.h = d.h >= 0 ? h->slot(d.h) : nullptr;
        g.xout = d.xout >= 0 ? h->slot(d.xout) : nullptr;
        a.tile_start[ns] = tile;
        tile += g.n_tiles;
        ++ns;
    }
    a.nseg = ns;
    a.tile_start[ns] = tile;
    *out = a;
    *K = sd.K;
    return WRNN_OK;
}

int launch_step(wrnn_handle* h, int t, int S, bool timing) {
    hipStream_t st = h->stream;
    for (size_t si = 0; si < h->stages.size(); ++si) {
        StageArgs a;
        int K;
        CHECK(build_stage_args(h, (int)si, t, S, timing, &a, &K));
        HIPC(launch_stage(a, K, h->RT, h->nrg, h->nrt, st));
    }
    SampleArgs sa{};
    sa.t = t;
    sa.S = h->ws.S;  // row stride of labels/samples = capacity
    sa.nrows = h->last_B;
    sa.n_classes = h->n_classes;
    sa.mode = h->cfg.mode;
    sa.H = h->H;
    sa.logits = h->slot(SL_LOG);
    sa.noise = nullptr;
    sa.samples = h->ws.samples.f();
    sa.labels = (int16_t*)h->ws.labels.p;
    sa.do_gru = t + 1 < S;
    sa.P1 = h->slot(SL_P1);
    sa.v = h->v1;
    sa.gh1 = h->slot(SL_GH1);
    sa.h1 = h->slot(SL_H1);
    sa.x1 = h->slot(SL_X1);
    sa.cI = h->ws.cI.f();
    sa.w0 = h->w0;
    sa.rows = (const RowInfo*)h->ws.rows.p;
    sa.k0 = (uint32_t)(h->seed & 0xffffffffu);
    sa.k1 = (uint32_t)(h->seed >> 32);
    sa.phases = nullptr;
    sa.dbg = h->dbg;
    if (t == h->phase_step && h->phases.p)
        sa.phases = (uint32_t*)h->phases.p + h->stages.size() * kMaxStampWG * 8;
    HIPC(launch_sample(sa, st));
    return WRNN_OK;
}

void phase_report(wrnn_handle* h) {
    const int ns = (int)h->stages.size();
    std::vector<uint32_t> ph((size_t)(ns + 1) * kMaxStampWG * 8);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return;
    if (hipMemcpy(ph.data(), h->phases.p, ph.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return;
    const int t = h->phase_step;
    for (int s = 0; s <= ns; ++s) {
        int nwg, nph;
        if (s < ns) {
            StageArgs a;
            int K;
            if (build_stage_args(h, s, t, h->last_S, false, &a, &K)) return;
            nwg = std::min(kMaxStampWG, a.tile_start[a.nseg] * h->nrt);
            nph = 5;
        } else {
            nwg = h->last_B;
            nph = 3;
        }
        const uint32_t* p = ph.data() + (size_t)s * kMaxStampWG * 8;
        long long t0 = 0;
        bool first = true;
        for (int w = 0; w < nwg; ++w) {
            const long long v = (long long)p[8 * w];
            if (first || v < t0) t0 = v;
            first = false;
        }
        std::fprintf(stderr, "[wrnn phases] step %d %-6s wg=%4d", t,
                     s < ns ? h->stages[s].name.c_str() : "sample", nwg);
        for (int i = 0; i < nph; ++i) {
            std::vector<double> d;
            for (int w = 0; w < nwg; ++w) d.push_back(((long long)p[8 * w + i] - t0) * 0.01);
            std::sort(d.begin(), d.end());
            std::fprintf(stderr, "  p%d med %.2f max %.2f", i, d[d.size() / 2], d.back());
        }
        std::fprintf(stderr, " (us)\n");
    }
}

// A noise-seed-dependent kernel argument (MOL Philox key) is baked into captured graphs, so the
// cache key includes it through `timing` only when RAW; MOL / BETA graphs are keyed by seed below.
int run_chunk(wrnn_handle* h, int t0, int len, int S) {
    const bool last = t0 + len >= S;
    const int key_S = last ? S : -1;
    auto key = std::make_tuple(t0, len, key_S, h->last_B,
                               (h->timing ? 1 : 0) | ((h->phase_step + 1) << 1),
                               h->cfg.mode != WRNN_MODE_RAW ? h->seed : (uint64_t)0, h->dbg_gen);
    auto it = h->graphs.find(key);
    if (it == h->graphs.end()) {
        hipGraph_t g;
        HIPC(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
        int rc = WRNN_OK;
        for (int t = t0; t < t0 + len && rc == WRNN_OK; ++t) rc = launch_step(h, t, S, h->timing);
        hipError_t e = hipStreamEndCapture(h->stream, &g);
        if (rc != WRNN_OK) return rc;
        HIPC(e);
        hipGraphExec_t ge;
        hipError_t ei = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        HIPC(ei);
        it = h->graphs.emplace(key, ge).first;
    }
    HIPC(hipGraphLaunch(it->second, h->stream));
    return WRNN_OK;
}

void fold_shape(int L, int batched, int target, int overlap, int* B, int* S) {
    if (!batched) {
        *B = 1;
        *S = L;
        return;
    }
    int nf = (L - overlap) / (target + overlap);
    const int ext = nf * (overlap + target) + overlap;
    if (L - ext != 0) nf += 1;
    *B = nf;
    *S = target + 2 * overlap;
}

struct UttPlan {
    int T, L, B, Lpad, pbase, fbase, row0;
    int f0;  // first fold row of the call (wrnn_set_fold_ranges; 0 otherwise)
};

// CHAIN engine: per step one launch per stage + the sampler, captured 100 steps per graph.
int run_chain(wrnn_handle* h, int S, wrnn_progress_fn cb, void* user) {
    auto& ws = h->ws;
    const int B = h->last_B;
    h->RT = pick_rt(B, &h->nrt);
    for (const StageDesc& sd : h->stages) HIPC(prepare_stage(sd.K, h->RT, h->nrg));
    {
        const char* env = std::getenv("WRNN_PHASE_STEP");
        h->phase_step = env ? std::atoi(env) : -1;
        if (h->phase_step >= S) h->phase_step = S - 1;
        if (h->phase_step >= 0 && !h->phases.p)
            CHECK(h->phases.alloc((h->stages.size() + 1) * kMaxStampWG * 8 * sizeof(uint32_t)));
    }
    // initial state: h = 0, gh = b_hh, then P1(0) and GRU1 of step 0
    const int ngru = h->n_gru;
    for (int g = 0; g < ngru; ++g) {
        HIPC(launch_fill_rows(h->slot(SL_H1 + g), nullptr, h->H, B, h->stream));
        HIPC(launch_fill_rows(h->slot(SL_GH1 + g), h->dvec["rnn" + std::to_string(g + 1) + ".bias_hh_l0"],
                              3 * h->H, B, h->stream));
    }
    {
        // P1 for step 0: the stage holding the SL_CI segment, run with t = -1 (x_off = 0)
        for (size_t si = 0; si < h->stages.size(); ++si) {
            const StageDesc& sd = h->stages[si];
            for (const SegDesc& d : sd.segs)
                if (d.x == SL_CI) {
                    StageArgs a{};
                    int K;
                    CHECK(build_stage_args(h, (int)si, -1, S, false, &a, &K));
                    // keep only the SL_CI segment
                    for (int k = 0; k < a.nseg; ++k)
                        if (a.seg[k].X == ws.cI.f()) {
                            StageArgs b = a;
                            b.seg[0] = a.seg[k];
                            b.nseg = 1;
                            b.tile_start[0] = 0;
                            b.tile_start[1] = a.seg[k].n_tiles;
                            HIPC(launch_stage(b, K, h->RT, h->nrg, h->nrt, h->stream));
                        }
                }
        }
        SampleArgs sa{};
        sa.t = -1;
        sa.S = ws.S;
        sa.nrows = B;
        sa.n_classes = h->n_classes;
        sa.mode = h->cfg.mode;
        sa.H = h->H;
        sa.do_gru = 1;
        sa.P1 = h->slot(SL_P1);
        sa.v = h->v1;
        sa.gh1 = h->slot(SL_GH1);
        sa.h1 = h->slot(SL_H1);
        sa.x1 = h->slot(SL_X1);
        sa.cI = ws.cI.f();
        sa.w0 = h->w0;
        sa.rows = (const RowInfo*)ws.rows.p;
        HIPC(launch_sample(sa, h->stream));
    }
    for (const StageDesc& sd : h->stages) HIPC(prepare_stage(sd.K, h->RT, h->nrg));
    if (h->timing) {
        const size_t need = ((size_t)S / kStampEvery + 1) * h->stages.size() * kMaxStampWG * 2 *
                            sizeof(uint32_t);
        if (need > ws.stamps.bytes) {
            for (auto& kv : h->graphs) (void)hipGraphExecDestroy(kv.second);
            h->graphs.clear();
            ws.stamps.release();
            CHECK(ws.stamps.alloc(need));
        }
        HIPC(hipMemsetAsync(ws.stamps.p, 0, need, h->stream));
    }
    // the recurrence, 100 steps per graph (progress granularity of the reference)
    const int G = 100;
    const auto t_start = std::chrono::steady_clock::now();
    std::vector<hipEvent_t> evs;
    int rc = WRNN_OK;
    const int nchunks = (S + G - 1) / G;
    evs.resize(nchunks, nullptr);
    for (int c = 0; c < nchunks && rc == WRNN_OK; ++c) {
        const int t0 = c * G, len = std::min(G, S - t0);
        rc = run_chunk(h, t0, len, S);
        if (rc) break;
        if (cb) {
            if (hipEventCreateWithFlags(&evs[c], hipEventDisableTiming) != hipSuccess ||
                hipEventRecord(evs[c], h->stream) != hipSuccess) {
                rc = fail(WRNN_ERR_HIP, "event record");
                break;
            }
            // report the previous chunk once it is done (keeps one chunk queued ahead)
            if (c >= 1) {
                (void)hipEventSynchronize(evs[c - 1]);
                const int i = (c - 1) * G;
                const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
                const double rate = (i + 1) / std::max(el, 1e-9) * B / 1000.0;
                if (cb(user, i, S, B, rate)) rc = fail(WRNN_ERR_ABORTED, "aborted by progress callback");
            }
        }
    }
    if (rc == WRNN_OK && cb && nchunks >= 1) {
        (void)hipEventSynchronize(evs[nchunks - 1]);
        const int i = (nchunks - 1) * G;
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
        if (cb(user, i, S, B, (i + 1) / std::max(el, 1e-9) * B / 1000.0))
            rc = fail(WRNN_ERR_ABORTED, "aborted by progress callback");
    }
    for (auto e : evs)
        if (e) (void)hipEventDestroy(e);
    if (rc) return rc;
    if (h->phase_step >= 0) phase_report(h);
    return WRNN_OK;
}

constexpr int kPersistFallback = 1;  // internal: retry the call on the CHAIN engine
constexpr int kPersistMaxStreak = 3; // consecutive failed persistent calls before AUTO stops trying

bool persist_device_ok(wrnn_handle* h) {
    static int cached[64];  // 0 unknown, 1 ok, 2 not ok (per device ordinal)
    const int d = h->device;
    if (d >= 0 && d < 64 && cached[d]) return cached[d] == 1;
    hipDeviceProp_t p;
    bool ok = hipGetDeviceProperties(&p, d) == hipSuccess && p.multiProcessorCount == kPG * kPM &&
              std::strncmp(p.gcnArchName, "gfx950", 6) == 0 &&
              p.sharedMemPerMultiprocessor >= std::max({persist_lds_bytes(), persist_rr_lds_bytes(),
                                                        persist_gen_lds_bytes(), persist_wide_lds_bytes(),
                                                        persist_wide_sp_lds_bytes()});
    if (d >= 0 && d < 64) cached[d] = ok ? 1 : 2;
    return ok;
}

void persist_phase_report(wrnn_handle* h, int t) {
    // per group: the last workgroup to reach each phase (the group's critical path), relative
    // to the group's first start; printed as the median and max over the 8 groups
    std::vector<uint32_t> ph((size_t)kPG * kPM * kPPhases);
    if (hipStreamSynchronize(h->stream) != hipSuccess) return;
    if (hipMemcpy(ph.data(), h->pws.phases.p, ph.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return;
    static const char* names[] = {"start", "A", "hopA", "B", "hopB", "C", "hopC", "D", "hopD", "sample", "gru1", "fc3"};
    std::fprintf(stderr, "[wrnn persist phases] step %d: last workgroup of each group, us from the group's first start"
                         " (wave 0 | wave 4)\n", t);
    for (int i = 0; i < 12; ++i) {
        double med[2] = {0, 0}, mxx[2] = {0, 0};
        for (int wv = 0; wv < 2; ++wv) {
            std::vector<double> d;
            for (int g = 0; g < kPG; ++g) {
                long long t0 = -1, mx = -1;
                for (int w = 0; w < kPM; ++w) {
                    const uint32_t s0 = ph[((size_t)g * kPM + w) * kPPhases];
                    const uint32_t v = ph[((size_t)g * kPM + w) * kPPhases + 12 * wv + i];
                    if (s0 && (t0 < 0 || s0 < t0)) t0 = s0;
                    if (v && (long long)v > mx) mx = v;
                }
                if (t0 >= 0 && mx >= 0) d.push_back((mx - t0) * 0.01);
            }
            if (d.empty()) continue;
            std::sort(d.begin(), d.end());
            med[wv] = d[d.size() / 2];
            mxx[wv] = d.back();
        }
        // and each workgroup's own timeline (from its own start), median over all workgroups
        std::vector<double> own;
        for (int gw = 0; gw < kPG * kPM; ++gw) {
            const uint32_t s0 = ph[(size_t)gw * kPPhases], v = ph[(size_t)gw * kPPhases + i];
            if (s0 && v) own.push_back(((long long)v - (long long)s0) * 0.01);
        }
        std::sort(own.begin(), own.end());
        std::fprintf(stderr, "  %-7s med %6.2f max %6.2f | med %6.2f max %6.2f | own wave 0 %6.2f\n", names[i],
                     med[0], mxx[0], med[1], mxx[1], own.empty() ? 0.0 : own[own.size() / 2]);
    }
    // optional extra wave-0 stamps at [26, 32) (kernel experiments), own timeline
    for (int i = 26; i < kPPhases; ++i) {
        std::vector<double> own;
        for (int gw = 0; gw < kPG * kPM; ++gw) {
            const uint32_t s0 = ph[(size_t)gw * kPPhases], v = ph[(size_t)gw * kPPhases + i];
            if (s0 && v) own.push_back(((long long)v - (long long)s0) * 0.01);
        }
        if (own.empty()) continue;
        std::sort(own.begin(), own.end());
        std::fprintf(stderr, "  x%-6d own wave 0 med %6.2f max %6.2f\n", i, own[own.size() / 2], own.back());
    }
    {
        // core clock of workgroup 0: shader cycles / 100 MHz ticks over the traced step
        const double cyc = (double)(uint32_t)(ph[25] - ph[24]);
        const double us = ((long long)ph[10] - (long long)ph[0]) * 0.01;
        if (us > 0) std::fprintf(stderr, "  shader clock ~ %.0f MHz\n", cyc / us);
    }
}

// Phase stamps of the runtimeracer wide kernel (kernels_persist_wide_rr.hip RS): wave 0 of
// slot 0 (half A) and slot 16 (half B) of every group, us from A's step start, median over groups.
void persist_wide_rr_phase_report(wrnn_handle* h, int t) {
    std::vector<uint32_t> ph((size_t)kPG * kPM * kPPhases);
    if (hipMemcpy(ph.data(), h->pws.phases.p, ph.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return;
    static const char* na[] = {"top", "x1 poll", "W_ih2 x1", "x2 pub", "h2 poll", "W_hh2 h2", "x3 poll",
                               "x4 pub", "W_hh4 h4", "y1 poll", "y2 pub", "y3 poll", "y4 pub", "ring"};
    static const char* nb[] = {"top", "h1 poll", "W_hh1 h1", "x2 poll", "x3 pub", "W_hh3 h3", "x4 poll",
                               "y1 pub", "y2 poll", "y3 pub", "y4 poll", "fc5", "cand pub", "sample", "x1 pub"};
    std::fprintf(stderr, "[wrnn persist-wide-rr phases] step %d: slot 0 (A) / slot 16 (B), us from A's step start, median over groups\n", t);
    for (int half = 0; half < 2; ++half) {
        const int n = half ? 15 : 14;
        for (int i = 0; i < n; ++i) {
            std::vector<double> d;
            for (int g = 0; g < kPG; ++g) {
                const uint32_t t0 = ph[(size_t)(g * kPM + 0) * kPPhases];
                const uint32_t v = ph[(size_t)(g * kPM + 16 * half) * kPPhases + i];
                if (t0 && v) d.push_back(((long long)v - (long long)t0) * 0.01);
            }
            if (d.empty()) continue;
            std::sort(d.begin(), d.end());
            std::fprintf(stderr, "  %s %-9s med %6.2f max %6.2f\n", half ? "B" : "A", half ? nb[i] : na[i],
                         d[d.size() / 2], d.back());
        }
    }
}

// PERSIST engine: P1 for all steps (one MFMA GEMM), Gumbel noise (RAW), step-0 state, then
// the persistent recurrence in chunks (one chunk per call unless a progress callback wants
// reports; every 1000 steps then).
// Gumbel (RAW) / MOL noise of every (step, row) of the call on stream `st` (the RNG contract).
int persist_noise(wrnn_handle* h, int S, hipStream_t st) {
    auto& P = h->pws;
    const int Bp = h->last_Bp, n = h->n_classes;
    const bool raw = h->cfg.mode == WRNN_MODE_RAW;
    if (h->cfg.mode == WRNN_MODE_BETA) {  // gamma draws are made in-kernel
        CHECK(P.gumbel.alloc(sizeof(float)));
        return WRNN_OK;
    }
    // rows that need the stream: the register-resident launches' (k_persist forming its noise
    // in-kernel measured 6.52 against 5.93 us per C2 step, DESIGN §3.0: the stream stays)
    bool any_wide = false, any_reg = false;
    for (const auto& L : h->p_plan) {
        any_wide |= L.wide;
        any_reg |= !L.wide;
    }
    // (a rotated plan has only register-resident launches over the same rows: any_wide false)
    // (the geneing wide kernel's stream instances read the stream like k_persist_gen: the whole
    // stream below; its ring instances, in calls of wide launches only, draw in-kernel)
    const bool ring_noise = any_wide && (!h->pw.gen || h->gen_ring);
    if (raw && ring_noise && !any_reg) {  // every launch draws its noise in-kernel
        CHECK(P.gumbel.alloc(sizeof(float)));
        return WRNN_OK;
    }
    CHECK(P.gumbel.alloc((size_t)S * Bp * (raw ? n : kMolNoise) * sizeof(float)));
    const uint32_t k0 = (uint32_t)(h->seed & 0xffffffffu), k1 = (uint32_t)(h->seed >> 32);
    const RowInfo* rows = (const RowInfo*)h->ws.rows.p;
    if (raw && ring_noise) {
        // the wide launches draw their noise in-kernel (kernels_persist_wide.hip ring): fill
        // only the rows of the register-resident launches (C4: 16 of 144 rows, 3.6 -> 0.4 ms)
        for (const auto& L : h->p_plan)
            if (!L.wide) HIPC(launch_gumbel_rows(P.gumbel.f(), S, L.rb, kPG * L.nr, Bp, n, rows, k0, k1, st));
    } else if (raw) {
        HIPC(launch_gumbel(P.gumbel.f(), S, Bp, n, rows, k0, k1, st));
    } else {
        HIPC(launch_mol_noise(P.gumbel.f(), S, Bp, rows, k0, k1, st));
    }
    return WRNN_OK;
}

int run_persist(wrnn_handle* h, int S, wrnn_progress_fn cb, void* user) {
    auto& ws = h->ws;
    auto& P = h->pws;
    const auto& W = h->pw;
    const int B = h->last_B, Bp = h->last_Bp, H = kPH, n = h->n_classes;  // H: fatchord layout
    hipStream_t st = h->stream;
    CHECK(P.ctl.alloc(PC_WORDS * sizeof(unsigned)));
    const bool rr = W.rr, gen = W.gen;
    bool any_wide = false;
    bool any32 = false;  // geneing launches of more than 16 rows per group (two column tiles)
    for (const auto& L : h->p_plan) {
        any_wide |= L.wide;
        any32 |= gen && L.wide && L.nr > kPWideRows;
    }
    const size_t xfl = gen  ? std::max(persist_gen_xbuf_floats(), any32      ? persist_wide_gen32_xbuf_floats()
                                                                  : any_wide ? persist_wide_gen_xbuf_floats() : 0)
                       : rr ? std::max(persist_rr_xbuf_floats(), any_wide ? persist_wide_rr_xbuf_floats() : 0)
                            : std::max(persist_xbuf_floats(), any_wide ? persist_wide_xbuf_floats() : 0);
    CHECK(P.xbuf.alloc(xfl * sizeof(float)));
    CHECK(P.st.alloc((size_t)Bp * (gen ? 2 * kRH : rr ? kRRState * kRH : 6 * H) * sizeof(float)));
    // P1 (all steps, rows) was written by run_upsample next to cI; the noise by
    // persist_noise on the side stream
    const uint32_t k0 = (uint32_t)(h->seed & 0xffffffffu), k1 = (uint32_t)(h->seed >> 32);
    if (h->noise_pending) {
        HIPC(hipStreamWaitEvent(st, h->noise_done, 0));
        h->noise_pending = false;
    } else {
        CHECK(persist_noise(h, S, st));
    }
    PersistArgs a{};
    a.ctl = (unsigned*)P.ctl.p;
    a.xbuf = P.xbuf.f();
    a.S = S;
    a.B = Bp;
    a.nreal = B;
    a.nr = Bp / kPG;
    a.mode = h->cfg.mode;
    a.n_classes = n;
    a.hop = h->hop;
    a.cpw = W.cpw;
    a.rows = (const RowInfo*)ws.rows.p;
    a.wreg = (const float4*)(h->sparse_call ? W.swreg : W.wreg);
    a.wlds = (const float4*)(h->sparse_call ? W.swlds : W.wlds);
    a.sparse = h->sparse_call ? 1 : 0;
    a.b_hh1 = W.b_hh1;
    a.b_hh2 = W.b_hh2;
    a.b_fc3 = W.b_fc3;
    a.v = h->v1;
    a.w0 = h->w0;
    a.fcond = ws.fcond.f();
    a.cond_width = h->cond_width;
    a.oG2 = W.oG2;
    a.oF1 = W.oF1;
    a.oF2 = W.oF2;
    a.P1 = P.P1.f();
    a.cI = ws.cI.f();
    if (h->p1_ring && !rr && !gen) {  // k_persist and k_persist_wide form P1 in-kernel
        a.p1q = ws.q4.f();
        a.p1a = ws.a4.f();
        a.p1taps = W.p1taps + (size_t)h->hop * 8;  // the [hop][4] table
        a.p1split = W.p1split;
    }
    a.gumbel = P.gumbel.f();
    a.dbg = h->dbg;
    a.labels = (int16_t*)ws.labels.p;
    a.samples = ws.samples.f();
    a.ld = ws.S;
    a.k0 = k0;
    a.k1 = k1;
    a.st_x1 = P.st.f();
    a.st_h1 = a.st_x1 + (size_t)Bp * H;
    a.st_h2 = a.st_h1 + (size_t)Bp * H;
    a.st_gh2 = a.st_h2 + (size_t)Bp * H;
    a.phase_t = -1;
    if (const char* env = std::getenv("WRNN_PHASE_STEP")) {
        a.phase_t = std::min(std::atoi(env), S - 1);
        CHECK(P.phases.alloc((size_t)kPG * kPM * kPPhases * sizeof(uint32_t)));
        HIPC(hipMemsetAsync(P.phases.p, 0, P.phases.bytes, st));
        a.phases = (uint32_t*)P.phases.p;
    }
    PersistGenArgs ag{};
    PersistRRArgs ar{};
    if (gen) {
        ag.ctl = a.ctl;
        ag.xbuf = a.xbuf;
        ag.S = S;
        ag.B = Bp;
        ag.mode = a.mode;
        ag.n_classes = n;
        ag.hop = a.hop;
        ag.cpw = W.cpw;
        ag.rows = a.rows;
        ag.wreg = (const float4*)W.wreg;
        ag.b_hh1 = W.b_hh1;
        ag.b_f3 = W.b_fc3;
        ag.v = h->v1;
        ag.w0 = h->w0;
        ag.fcond = a.fcond;
        ag.cond_width = a.cond_width;
        ag.oF1 = W.oF1;
        ag.P1 = a.P1;
        ag.cI = a.cI;
        ag.gumbel = a.gumbel;
        ag.labels = a.labels;
        ag.samples = a.samples;
        ag.ld = a.ld;
        ag.st = P.st.f();
        ag.k0 = (uint32_t)(h->seed & 0xffffffffu);
        ag.k1 = (uint32_t)(h->seed >> 32);
        ag.dbg = h->dbg;
        ag.wwide = (const float4*)W.wwide_gen;
        HIPC(launch_persist_gen_init(ag, st));
    } else if (rr) {
        ar.ctl = a.ctl;
        ar.xbuf = a.xbuf;
        ar.S = S;
        ar.B = Bp;
        ar.mode = a.mode;
        ar.n_classes = n;
        ar.hop = a.hop;
        ar.cpw = W.cpw;
        ar.rows = a.rows;
        ar.wreg = (const float4*)W.wreg;
        ar.w5 = (const float4*)W.wlds;
        ar.b_ih2 = W.b_ih2;
        ar.b_ih4 = W.b_ih4;
        ar.b_hh1 = W.b_hh1;
        ar.b_hh2 = W.b_hh2;
        ar.b_hh3 = W.b_hh3;
        ar.b_hh4 = W.b_hh4;
        ar.b_f2 = W.b_f2;
        ar.b_f4 = W.b_f4;
        ar.b_f5 = W.b_fc3;
        ar.v = h->v1;
        ar.w0 = h->w0;
        ar.fcond = a.fcond;
        ar.cond_width = a.cond_width;
        ar.oG3 = W.oG2;
        ar.oF1 = W.oF1;
        ar.oF3 = W.oF2;
        ar.P1 = a.P1;
        ar.cI = a.cI;
        ar.gumbel = a.gumbel;
        ar.labels = a.labels;
        ar.samples = a.samples;
        ar.ld = a.ld;
        ar.st = P.st.f();
        ar.dbg = h->dbg;
        HIPC(launch_persist_rr_init(ar, st));
    } else {
        HIPC(launch_persist_init(a, st));
    }
    HIPC(hipMemsetAsync(P.ctl.p, 0, PC_WORDS * sizeof(unsigned), st));
    if (const char* inj = std::getenv("WRNN_DEBUG_PERSIST_FAIL"); inj && std::strcmp(inj, "occupancy")) {
        // test hook: the call's launches find a co-residency error already set at registration
        // and exit, exercising the real failure path (fallback / error, warning, counters)
        static const unsigned kInjected = 1u;
        HIPC(hipMemcpyAsync((unsigned*)P.ctl.p + PC_ERR, &kInjected, sizeof(unsigned), hipMemcpyHostToDevice, st));
    }
    // launches: one per row batch, each running all S steps; the step tags restart with every
    // batch, so the exchange area is cleared before each. A progress callback does
    // not split launches: the kernels publish their step count to a host-mapped word every 100
    // steps (persist_common.h p_progress) and this thread reports from it while they run.
    const int nb = (int)h->p_plan.size();
    a.wwide = (const float4*)W.wwide;
    a.wwide_lds = (const float4*)W.wwide_lds;
    a.wfc3b = (const float4*)W.wfc3b;
    if (any_wide && !gen) {  // the wide kernels form P1 and the noise in-kernel into this ring
        CHECK(P.wring.alloc((rr ? persist_wide_rr_ring_floats() : persist_wide_ring_floats()) * sizeof(float)));
        a.wring = P.wring.f();
        ar.wring = a.wring;
        ar.wwide = (const float4*)W.wwide_rr;
        if (rr && rr_frames_ok(h)) {
            ar.p1q = ws.q4.f();
            ar.p1a = ws.a4.f();
            ar.p1taps = W.p1taps + (size_t)h->hop * 8;  // the [hop][4] table
            ar.p1split = W.p1split;
        }
        ar.k0 = k0;
        ar.k1 = k1;
    }
    ar.phases = a.phases;
    ar.phase_t = a.phase_t;
    if (cb && !h->prog_host) {  // progress word + abort word (kAbortWord), two cache lines
        HIPC(hipHostMalloc((void**)&h->prog_host, 128, hipHostMallocMapped | hipHostMallocCoherent));
        HIPC(hipHostGetDevicePointer((void**)&h->prog_dev, h->prog_host, 0));
    }
    if (cb) {
        __atomic_store_n(h->prog_host, 0u, __ATOMIC_RELAXED);
        __atomic_store_n(h->prog_host + kAbortWord, 0u, __ATOMIC_RELAXED);
    }
    a.progress = ag.progress = ar.progress = cb ? h->prog_dev : nullptr;
    for (auto e : h->pev) (void)hipEventDestroy(e);
    h->pev.clear();
    h->pev_steps.clear();
    h->pev_kind.clear();
    h->pev_rows.clear();
    if (h->timing) CHECK(P.stamps.alloc((size_t)nb * 2 * sizeof(uint32_t)));
    // row rotation: per launch j the virtual-row map, rows / steps per group and the RowInfo
    // table by virtual row (rel0 advanced by the row's offset), one device block per launch
    const auto& RP = h->rot_plan;
    // (register-resident rotation or time-sliced wide launches): per launch j the virtual-row map,
    // for the rotation the rows and steps per group, and the RowInfo table by virtual row (rel0
    // advanced by the row's offset) -- one device block per launch
    const bool rotp = nb > 0 && h->p_plan[0].rot >= 0;
    std::vector<size_t> rot_off;  // per launch: byte offset of its block
    if (rotp) {
        // a rotated launch's block holds kPG * nr_hi row slots and the kernel runs L.nr rows:
        // they must agree (generate_impl plans the rotation only then)
        for (const auto& L : h->p_plan)
            if (!L.wide && L.nr != RP.nr_hi)
                return fail(WRNN_ERR_INVALID, "rotated launch with " + std::to_string(L.nr) +
                                                   " rows per group, rotation plan of " + std::to_string(RP.nr_hi));
        auto nv_of = [&](const PLaunch& L) { return kPG * (L.wide ? h->wrot[L.rot].nr : RP.nr_hi); };
        size_t total = 0;
        for (const auto& L : h->p_plan) {
            rot_off.push_back(total);
            const int nv = nv_of(L);
            total += ((size_t)nv * (sizeof(int2) + sizeof(RowInfo)) + 2 * kPG * sizeof(int) + 255) & ~(size_t)255;
        }
        h->rot_host.assign(total, 0);
        for (int b = 0; b < nb; ++b) {
            const auto& L = h->p_plan[b];
            const int nv = nv_of(L);
            char* base = h->rot_host.data() + rot_off[b];
            const VRow* vm = L.wide ? h->wrot[L.rot].vmap.data() : &RP.vmap[(size_t)L.rot * nv];
            // the kernels read the planner's maps as int2 (row = x, off = y)
            static_assert(sizeof(VRow) == sizeof(int2) && offsetof(VRow, row) == offsetof(int2, x) &&
                              offsetof(VRow, off) == offsetof(int2, y),
                          "VRow must have int2's layout");
            std::memcpy(base, vm, (size_t)nv * sizeof(int2));
            int* gi = reinterpret_cast<int*>(base + (size_t)nv * sizeof(int2));
            if (!L.wide) {
                std::memcpy(gi, &RP.gnr[(size_t)L.rot * kPG], kPG * sizeof(int));
                std::memcpy(gi + kPG, &RP.git[(size_t)L.rot * kPG], kPG * sizeof(int));
            }
            RowInfo* rv = reinterpret_cast<RowInfo*>(gi + 2 * kPG);
            for (int v = 0; v < nv; ++v) {
                rv[v] = h->rows_host[vm[v].row];
                rv[v].rel0 += vm[v].off;
            }
        }
        CHECK(P.rot.alloc(h->rot_host.size()));
        HIPC(hipMemcpyAsync(P.rot.p, h->rot_host.data(), h->rot_host.size(), hipMemcpyHostToDevice, st));
    }
    const auto t_start = std::chrono::steady_clock::now();
    // time-sliced wide launches publish their progress on a common scale: launch b starts at the
    // steps of the launches before it (prog_base), the host maps the total to 0 .. S
    const bool wsl = nb > 0 && h->p_plan[0].wide && h->p_plan[0].rot >= 0;
    long long sl_total = 0;
    if (wsl)
        for (const auto& L : h->p_plan) sl_total += h->wrot[L.rot].steps;
    long long sl_cum = 0;
    for (int b = 0; b < nb; ++b) {
        const auto& L = h->p_plan[b];
        a.rb = L.rb;
        a.nr = L.nr;
        a.t0 = 0;
        a.t1 = S;
        a.prog_base = wsl ? (int)sl_cum : b * S;
        if (wsl) sl_cum += h->wrot[L.rot].steps;
        a.vmap = nullptr;
        a.gnr = a.giters = nullptr;
        a.rows = (const RowInfo*)ws.rows.p;
        double steps_b = S;  // (this launch's steps, for the per-launch accounting)
        if (L.rot >= 0) {
            const char* base = (const char*)P.rot.p + rot_off[b];
            const int nv = kPG * L.nr;
            a.vmap = (const int2*)base;
            a.rows = (const RowInfo*)(base + (size_t)nv * sizeof(int2) + 2 * kPG * sizeof(int));
            if (L.wide) {
                a.t1 = h->wrot[L.rot].steps;
                steps_b = a.t1;
            } else {
                a.gnr = (const int*)(base + (size_t)nv * sizeof(int2));
                a.giters = a.gnr + kPG;
                a.t1 = std::max(RP.n_hi, RP.n_lo);
                steps_b = (double)S / RP.K;  // (per launch, on average: S per call)
            }
        }
        if (L.wide)  // sentinel-initialised vector slots (kernels_persist_wide*.hip polls)
            HIPC(gen  ? (L.nr > kPWideRows ? persist_wide_gen32_reset_xbuf(P.xbuf.f(), st)
                                           : persist_wide_gen_reset_xbuf(P.xbuf.f(), st))
                 : rr ? persist_wide_rr_reset_xbuf(P.xbuf.f(), st) : persist_wide_reset_xbuf(P.xbuf.f(), st));
        else
            HIPC(hipMemsetAsync(P.xbuf.p, 0, xfl * sizeof(float), st));  // step tags
        // registration words only: an error code from an earlier launch stays visible, so the
        // later launches of a failed call exit at registration (p_register)
        HIPC(hipMemsetAsync(P.ctl.p, 0, PC_ERR * sizeof(unsigned), st));
        a.stamps = h->timing ? (uint32_t*)P.stamps.p + 2 * b : nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (h->timing) {
            HIPC(hipEventCreate(&e0));
            HIPC(hipEventCreate(&e1));
            h->pev.push_back(e0);
            h->pev.push_back(e1);
            h->pev_steps.push_back(steps_b);
            h->pev_kind.push_back(L.sp ? 2 : L.wide ? 1 : 0);
            h->pev_rows.push_back(kPG * L.nr);
            HIPC(hipEventRecord(e0, st));
        }
        hipError_t le;
        if (gen) {
            ag.t0 = a.t0;
            ag.t1 = a.t1;
            ag.nr = a.nr;
            ag.rb = a.rb;
            ag.rows = a.rows;  // (a rotated launch: its own table, and the row map)
            ag.vmap = a.vmap;
            ag.gnr = a.gnr;
            ag.giters = a.giters;
            ag.stamps = a.stamps;
            ag.prog_base = a.prog_base;
            if (L.wide) {
                PersistGenArgs aw = ag;
                // classes per slot of the wide layout (BITS: every class owned, n = 32 cpw; MOL /
                // Beta: one tile of 16 in slots 0 and 1)
                aw.cpw = a.mode == WRNN_MODE_RAW ? n / kPM : 16;
                if (h->gen_ring) {  // the ring instances form P1 (BITS: and the noise) in-kernel
                    PersistGenRingArgs awr{};
                    static_cast<PersistGenArgs&>(awr) = aw;
                    awr.p1q = ws.q4.f();
                    awr.p1a = ws.a4.f();
                    awr.p1taps = W.p1taps + (size_t)h->hop * 8;  // the [hop][4] table
                    awr.p1split = W.p1split;
                    le = L.nr > kPWideRows ? launch_persist_wide_gen32_ring(awr, st)
                         : L.rot >= 0  ? launch_persist_wide_gen_rot(awr, st)  // time-sliced (its row map)
                                       : launch_persist_wide_gen_ring(awr, st);
                } else if (L.nr > kPWideRows) {
                    return fail(WRNN_ERR_INVALID, "32-row wide launch in a call with P1 / noise streams");
                } else {
                    le = launch_persist_wide_gen(aw, st);
                }
            } else if (h->gen_ring) {  // (plan_streams: the ring only in calls of wide launches)
                return fail(WRNN_ERR_INVALID, "register-resident launch in a call without P1 / noise streams");
            } else {
                le = launch_persist_gen(ag, st);
            }
        } else if (rr) {
            ar.t0 = a.t0;
            ar.t1 = a.t1;
            ar.nr = a.nr;
            ar.rb = a.rb;
            ar.rows = a.rows;  // (a time-sliced / rotated launch: its own table, and the row map)
            ar.vmap = a.vmap;
            ar.gnr = a.gnr;
            ar.giters = a.giters;
            ar.stamps = a.stamps;
            ar.prog_base = a.prog_base;
            if (L.wide) {
                PersistRRArgs aw = ar;
                // classes per B slot of the wide layout (16 slots per half; MOL: one tile of 16)
                aw.cpw = a.mode == WRNN_MODE_MOL ? 16 : n / 16;
                le = launch_persist_wide_rr(aw, st);
            } else {
                le = launch_persist_rr(ar, st);
            }
        } else if (L.sp) {  // block-sparse wide: the slots' list images in place of the MFMA tiles
            PersistArgs as = a;
            as.wwide_lds = (const float4*)W.wsp_img;
            le = launch_persist_wide_sp(as, st);
        } else if (L.wide) {
            le = launch_persist_wide(a, st);
        } else {
            le = launch_persist(a, st);
        }
        if (le == hipErrorCooperativeLaunchTooLarge) {
            // occupancy check of the launch wrapper: the grid cannot be co-resident, so the
            // launch was not made (no spinning); the call falls back / fails at once
            (void)hipStreamSynchronize(st);
            fail(WRNN_ERR_HIP, "persistent launch: workgroups cannot become co-resident (occupancy "
                               "check: fewer than 256 workgroups of 512 threads fit the device at once)");
            return kPersistFallback;
        }
        if (le != hipSuccess)
            return fail(WRNN_ERR_HIP, std::string("persistent launch: ") + hipGetErrorString(le));
        if (h->timing) HIPC(hipEventRecord(e1, st));
    }
    // the launches' error word is read only once they have finished (a copy into pageable
    // host memory queued here would block this thread until then, and every callback would
    // come after the fact)
    unsigned err = 0;
    auto read_err = [&]() -> hipError_t {
        return hipMemcpy(&err, (unsigned*)P.ctl.p + PC_ERR, sizeof(unsigned), hipMemcpyDeviceToHost);
    };
    int rc = WRNN_OK;
    if (cb) {
        // report i = 0, 100, 200, ... < S in order, each once, when every row has finished step i
        // (reference units: nb row batches of S steps make S steps of all B rows)
        hipEvent_t fin = nullptr;
        HIPC(hipEventCreateWithFlags(&fin, hipEventDisableTiming));
        if (hipEventRecord(fin, st) != hipSuccess) {
            (void)hipEventDestroy(fin);
            return fail(WRNN_ERR_HIP, "event record");
        }
        long long next = 0;
        while (rc == WRNN_OK && next < S) {
            const hipError_t q = hipEventQuery(fin);
            if (q != hipSuccess && q != hipErrorNotReady) {
                rc = fail(WRNN_ERR_HIP, std::string("persistent launch: ") + hipGetErrorString(q));
                break;
            }
            const bool finished = q == hipSuccess;
            if (finished) {
                if (read_err() != hipSuccess) {
                    rc = fail(WRNN_ERR_HIP, "persistent launch: reading its error word");
                    break;
                }
                if (err) break;  // failed launch: no progress to report
            }
            const long long done = finished ? (wsl ? sl_total : (long long)nb * S)
                                            : (long long)__atomic_load_n(h->prog_host, __ATOMIC_RELAXED);
            // steps every row has completed (sliced: the call's share of its row-steps, the
            // launches' step total scaled to S -- the rows advance in turns, so that is the
            // average row's step, reached by every row only at the end)
            const long long i_done = wsl ? done * S / std::max(1LL, sl_total) : done / nb;
            while (rc == WRNN_OK && next < S && next + 1 <= i_done) {
                const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
                if (cb(user, (int)next, S, B, (double)(next + 1) / std::max(el, 1e-9) * B / 1000.0)) {
                    // the reference stops at the raising step: ask the launches to drain
                    // (every group checks the word at its next progress point)
                    __atomic_store_n(h->prog_host + kAbortWord, 1u, __ATOMIC_RELAXED);
                    rc = fail(WRNN_ERR_ABORTED, "aborted by progress callback");
                }
                next += kProgressEvery;
            }
            if (!finished && next < S) std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
        (void)hipEventDestroy(fin);
    }
    HIPC(hipStreamSynchronize(st));
    if (rc) return rc;
    HIPC(read_err());
    if (err) {
        static const char* what[] = {"", "workgroups did not become co-resident",
                                     "exchange timeout", "workgroups not spread 32 per XCD",
                                     "aborted"};
        unsigned wh[3] = {0, 0, 0};
        (void)hipMemcpy(wh, (unsigned*)P.ctl.p + PC_WHERE, sizeof(wh), hipMemcpyDeviceToHost);
        const unsigned where = wh[0];
        if (where && std::getenv("WRNN_DEBUG_WHERE"))
            std::fprintf(stderr, "[wrnn] timeout detail: the timed-out poll's packets were %s\n",
                         wh[1] ? "missing" : "all present (a later check failed)");
        std::string msg = std::string("persistent launch: ") + (err < 5 ? what[err] : "unknown error");
        if (where)  // kernels_persist_wide.hip: the first timeout's site (PC_WHERE)
            msg += " (site " + std::to_string(where >> 28) +
                   ", slot " + std::to_string((where >> 22) & 31) + ", wave " + std::to_string((where >> 19) & 7) +
                   ", step " + std::to_string(wh[2]) + ")";
        fail(WRNN_ERR_HIP, msg);
        return kPersistFallback;
    }
    if (a.phase_t >= 0) {
        bool rr_wide = false;
        for (const auto& L : h->p_plan) rr_wide |= L.wide && rr;
        if (rr_wide) persist_wide_rr_phase_report(h, a.phase_t);
        else persist_phase_report(h, a.phase_t);
    }
    // algorithmic traffic per step: recurrent weights once + per row-step
    // conditioning (mel 80 + aux 128 floats) and the label
    // (every tensor of the step: I, rnn*, fc*; MACs: their weight matrices)
    double wparams = 0, macs = 0;
    for (const auto& kv : h->host) {
        const std::string& k = kv.first;
        if (k.rfind("I.", 0) && k.rfind("rnn", 0) && k.rfind("fc", 0)) continue;
        wparams += (double)kv.second.size();
        if (k.find("weight") != std::string::npos) macs += (double)kv.second.size();
    }
    // per launch kind (register-resident / wide): real rows averaged over its launches
    h->p_wbytes = 4.0 * wparams;
    h->p_row_bytes = (h->feat + h->R) * 4.0 + 2.0;
    h->p_macs = macs;
    if (h->sparse_call) {
        // sparse launches: the live blocks of the step matrices (16 B + a 2-byte index each)
        // replace their dense bytes / MACs; the rest (I, the aux columns, biases) unchanged
        double dense_k = 0;  // dense params of the matrices pack_persist_sparse lists
        dense_k = 3.0 * kPH * kPH * 3 + 2.0 * kPH * kPH + (double)h->n_classes * kPH;
        h->p_wbytes += W.sp_live_bytes - 4.0 * dense_k;
        h->p_macs += W.sp_live_macs - dense_k;
    }
    h->pstages.clear();
    for (const auto& L : h->p_plan) {
        int real = std::max(0, std::min(B, L.rb + kPG * L.nr) - L.rb);
        double steps = S;
        if (L.rot >= 0 && L.wide) steps = h->wrot[L.rot].steps;  // time-sliced: nr rows per group
        else if (L.rot >= 0) {                                    // rotation: all rows, S / K steps
            real = B;
            steps = (double)S / h->rot_plan.K;
        }
        const char* nm = L.sp ? "persist_wide_sp" : L.wide ? "persist_wide" : "persist";
        auto it = std::find_if(h->pstages.begin(), h->pstages.end(),
                               [&](const wrnn_handle::PStage& q) { return q.name == nm; });
        if (it == h->pstages.end()) {
            h->pstages.push_back({nm, L.sp ? 2 : L.wide ? 1 : 0, 0.0, 0});
            it = h->pstages.end() - 1;
        }
        it->rows += real;
        it->launches += 1;
        it->steps += steps;
        it->row_steps += steps * real;
    }
    return WRNN_OK;
}

// Captured CHAIN graphs are keyed by their launch arguments; those that hold buffers which
// are about to change are destroyed rather than kept unreachable.
static void drop_graphs(wrnn_handle* h) {
    for (auto& kv : h->graphs) (void)hipGraphExecDestroy(kv.second);
    h->graphs.clear();
}

// Logit capture of this call (wrnn_set_debug_steps): map[t] = slot of step t (or -1), the
// capture buffer NaN-filled so an unwritten entry shows. Off: null pointers in every launch.
int setup_debug_logits(wrnn_handle* h, int S, int Bp) {
    const bool on = !h->dbg_steps.empty();
    const void* out0 = h->dbg_out.p;
    const void* map0 = h->dbg_map.p;
    if (!on) {
        if (h->dbg.out) {
            ++h->dbg_gen;
            drop_graphs(h);  // graphs captured with capture buffers in their k_sample arguments
        }
        h->dbg = DbgLogits{};
        h->dbg_rows = 0;
        return WRNN_OK;
    }
    const size_t n_out = (size_t)kDbgSteps * Bp * h->n_classes;
    CHECK(h->dbg_out.alloc(n_out * sizeof(float)));
    CHECK(h->dbg_map.alloc((size_t)S * sizeof(int)));
    std::vector<int> map((size_t)S, -1);
    for (size_t k = 0; k < h->dbg_steps.size(); ++k)
        if (h->dbg_steps[k] < S) map[h->dbg_steps[k]] = (int)k;
    HIPC(hipMemcpyAsync(h->dbg_map.p, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPC(hipMemsetAsync(h->dbg_out.p, 0xff, n_out * sizeof(float), h->stream));  // NaN
    if (!h->dbg.out || out0 != h->dbg_out.p || map0 != h->dbg_map.p) {
        ++h->dbg_gen;
        drop_graphs(h);  // their k_sample arguments may hold the old capture buffers
    }
    h->dbg.out = h->dbg_out.f();
    h->dbg.map = (const int*)h->dbg_map.p;
    h->dbg_rows = Bp;
    h->dbg_S = S;
    return WRNN_OK;
}

// PlanIn of a call on this handle: variant scratch from the device code objects, env switches.
PlanIn plan_inputs(wrnn_handle* h, int B, int S) {
    PlanIn in;
    const auto& W = h->pw;
    in.ok = W.ok;
    in.rr = W.rr;
    in.gen = W.gen;
    in.fat = W.ok && !W.rr && !W.gen;
    in.mode = h->cfg.mode;
    in.n = h->n_classes;
    in.cpw = W.cpw;
    in.B = B;
    in.S = S;
    in.c10 = h->n_classes > kPM * 16;
    in.p1ring = p1_ring_ok(h);
    in.rr_frames = rr_frames_ok(h);
    // sparse k_persist instances (pruned checkpoints, §3.0g): when the model's image exists and
    // the call can form P1 in the ring; env WRNN_SPARSE=0 off (the dense kernels run the same
    // zeros to the same results)
    in.sp = in.fat && W.sp_ok && in.p1ring && (in.mode == WRNN_MODE_RAW || in.mode == WRNN_MODE_MOL);
    if (const char* e = std::getenv("WRNN_SPARSE")) {
        if (!std::strcmp(e, "0")) in.sp = false;
        if (!std::strcmp(e, "1")) in.force_sp = true;
    }
    // (the handle's mode is its head: wrnn_create admits Beta for geneing only)
    in.has_wide = (in.fat ? W.wwide : W.rr ? W.wwide_rr : W.gen ? W.wwide_gen : nullptr) != nullptr;
    if (!W.ok) return in;
    for (int c = 1; c <= kPNR; ++c) {
        if (in.fat) {
            in.scr[0][c] = persist_variant_scratch(c, W.cpw, in.mode, 0);
            in.scr[1][c] = persist_variant_scratch(c, W.cpw, in.mode, 1);
            in.scr_sp[c] = in.sp ? persist_variant_scratch(c, W.cpw, in.mode, 1, 1) : -1;
            in.scr_rot[0][c] = c >= 2 ? persist_rot_scratch(c, in.mode, 0) : -1;
            in.scr_rot[1][c] = c >= 2 && in.sp ? persist_rot_scratch(c, in.mode, 1) : -1;
        } else {
            in.ok_reg[c] = W.gen ? persist_gen_variant_ok(c, W.cpw, in.mode) != 0
                                 : persist_rr_variant_ok(c, W.cpw, in.mode) != 0;
            in.scr_rot[0][c] = c < 2 ? -1 : W.rr ? persist_rr_rot_scratch(c, in.mode == WRNN_MODE_MOL)
                                                 : persist_gen_rot_scratch(c, in.mode);
        }
    }
    const bool mol = in.mode == WRNN_MODE_MOL;
    if (in.has_wide && in.fat) {
        in.wide_scr = persist_wide_scratch(in.c10, mol);
        in.wide_rot_scr = persist_wide_rot_scratch(in.c10, mol);
    } else if (in.has_wide && W.rr) {
        in.wide_scr = persist_wide_rr_scratch(mol);
        in.wide_rot_scr = persist_wide_rr_rot_scratch(mol);
    } else if (in.has_wide) {
        in.wide_scr = persist_wide_gen_scratch(in.mode);
    }
    // block-sparse wide launches (§3.0g, the wide form): the image exists and both instances of
    // the class count run without scratch; env WRNN_SPARSE_WIDE=0|1 (read per call) forbids /
    // forces them, unset: by the rate keys wide and wide_sp
    in.has_wide_sp = in.has_wide && in.fat && in.mode == WRNN_MODE_RAW && W.wsp_img != nullptr &&
                     persist_wide_sp_scratch(false, in.c10) == 0 && persist_wide_sp_scratch(true, in.c10) == 0;
    if (const char* e = std::getenv("WRNN_SPARSE_WIDE")) {
        if (!std::strcmp(e, "0")) in.sp_wide_mode = 0;
        if (!std::strcmp(e, "1")) in.sp_wide_mode = 1;
    }
    if (const char* e = std::getenv("WRNN_PERSIST_WIDE")) in.wmode = std::atoi(e);
    if (const char* e = std::getenv("WRNN_PERSIST_NR_MAX")) in.nr_max = std::atoi(e);
    if (const char* e = std::getenv("WRNN_PERSIST_SLICE")) in.slice_off = !std::strcmp(e, "0");
    if (const char* e = std::getenv("WRNN_PERSIST_ROT")) in.rot_off = !std::strcmp(e, "0");
    in.allow_wide_scratch = std::getenv("WRNN_WIDE_ALLOW_SCRATCH") != nullptr;
    if (const char* e = std::getenv("WRNN_ROT_US")) std::sscanf(e, "%lf,%lf", &in.rot_hi, &in.rot_lo);
    return in;
}

int generate_impl(wrnn_handle* h, int n_utts, const float* const* mels, const int* n_frames,
                  int batched, int target, int overlap, int* row_offset, int* seq_len,
                  wrnn_progress_fn cb, void* user) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    // explicit per-utterance noise streams (wrnn_set_utt_streams) belong to this call whatever
    // its outcome: taken before any early return, so a failed call never leaves them armed for
    // an unrelated next one
    std::vector<uint32_t> ustreams;
    ustreams.swap(h->utt_streams);
    std::vector<int> flo, fhi;  // (wrnn_set_fold_ranges: likewise one call's)
    flo.swap(h->fold_lo);
    fhi.swap(h->fold_hi);
    if (!h->finalized)
        return fail(WRNN_ERR_NOT_LOADED, "Model hasn't been loaded. Call loadWeights first.");
    if (n_utts <= 0) return fail(WRNN_ERR_INVALID, "n_utts must be positive");
    if (batched && (target <= 0 || overlap < 0))
        return fail(WRNN_ERR_INVALID, "target must be > 0 and overlap >= 0");
    if (!flo.empty() && ((int)flo.size() != n_utts || !batched))
        return fail(WRNN_ERR_INVALID, !batched ? "fold ranges need a batched call"
                                               : "wrnn_set_fold_ranges gave " + std::to_string(flo.size()) +
                                                     " ranges for a call of " + std::to_string(n_utts) +
                                                     " utterances");
    std::vector<UttPlan> plan(n_utts);
    int B = 0, S = 0, P = 0, Fr = 0, Tmax = 0;
    for (int u = 0; u < n_utts; ++u) {
        UttPlan& p = plan[u];
        p.T = n_frames[u];
        if (p.T <= 0) return fail(WRNN_ERR_INVALID, "mel has no frames");
        p.L = p.T * h->hop;
        int b, s;
        fold_shape(p.L, batched, target, overlap, &b, &s);
        if (b <= 0) return fail(WRNN_ERR_INVALID, "mel too short for target/overlap");
        if (u && s != S)
            return fail(WRNN_ERR_INVALID, batched ? "inconsistent seq_len"
                                                  : "unbatched utterances of one call must have equal lengths");
        S = s;
        p.B = b;
        p.f0 = 0;
        p.Lpad = batched ? b * (target + overlap) + overlap : p.L;
        if (!flo.empty()) {  // a sub-range of the folds; positions stay those of the whole mel
            if (flo[u] < 0 || fhi[u] <= flo[u] || fhi[u] > b)
                return fail(WRNN_ERR_INVALID, "fold range [" + std::to_string(flo[u]) + ", " +
                                                  std::to_string(fhi[u]) + ") of utterance " + std::to_string(u) +
                                                  " outside its " + std::to_string(b) + " folds");
            p.f0 = flo[u];
            p.B = fhi[u] - flo[u];
        }
        p.pbase = P;
        // frame slots: [guard][zero frame = fbase][T frames][guard][guard], consecutive
        // utterances sharing one guard: the in-kernel P1 taps (frames f-2 .. f+2) then read
        // zero rows past either end without bounds checks
        p.fbase = Fr + 1;
        p.row0 = B;
        B += p.B;
        P += p.Lpad;
        Fr += p.T + 3;
        Tmax = std::max(Tmax, p.T);
    }
    if (B > 4096) return fail(WRNN_ERR_INVALID, "too many rows in one call (max 4096)");
    if (!ustreams.empty() && (int)ustreams.size() != n_utts)
        return fail(WRNN_ERR_INVALID, "wrnn_set_utt_streams gave " + std::to_string(ustreams.size()) +
                                          " streams for a call of " + std::to_string(n_utts) + " utterances");
    // engine: PERSIST when asked for / automatic and the call qualifies
    int want = h->engine;
    if (const char* env = std::getenv("WRNN_ENGINE")) {
        if (!std::strcmp(env, "chain")) want = WRNN_ENGINE_CHAIN;
        else if (!std::strcmp(env, "persist")) want = WRNN_ENGINE_PERSIST;
        else if (!std::strcmp(env, "auto")) want = WRNN_ENGINE_AUTO;
    }
    std::string why;
    // PERSIST launch plan (plan_call): register-resident and wide launches by the rates of
    // h->rates, then time-sliced wide launches or a row rotation
    PlanOut pout;
    PlanIn pin = plan_inputs(h, B, S);
    // geneing: the wide launches' ring instances (P1 and the BITS noise formed in-kernel) need the
    // per-frame P1 form, spill-free instances and frame tables inside one 2-GiB buffer range.
    // WRNN_GEN_RING=0|1 (read per call) forces the streams / the ring where it is possible
    int gen_ring_sw = -1;
    if (const char* env = std::getenv("WRNN_GEN_RING")) gen_ring_sw = std::atoi(env) != 0 ? 1 : 0;
    const bool gen_frames = h->pw.ok && h->pw.gen && h->pw.wwide_gen && h->pw.p1x4 && h->pw.p1taps_ok &&
                            h->pw.p1split >= 0 && p1_frames_enabled() &&
                            persist_wide_gen_ring_scratch(h->cfg.mode) == 0 &&
                            (double)(Fr + 1) * 4 * h->H * sizeof(float) < 2147483648.0;
    // 32-row launches (wrnn_set_gen_wide_rows, env WRNN_GEN_WIDE_ROWS=16|32 read per call): only
    // where the ring can be taken and the head's 32-row instance runs within its scratch rule
    int wide_rows = h->gen_wide_rows;
    if (const char* env = std::getenv("WRNN_GEN_WIDE_ROWS")) {
        const int v = std::atoi(env);
        if (v == kPWideRows || v == kPWideGen32Rows) wide_rows = v;
    }
    pin.gen32 = wide_rows == kPWideGen32Rows && gen_frames && gen_ring_sw != 0 &&
                persist_wide_gen32_usable(h->cfg.mode);
    // time-sliced launches (wrnn_set_gen_wide_slices, env WRNN_GEN_SLICE=0|1 read per call): under
    // the same conditions, for the head's time-sliced instance
    bool slices = h->gen_wide_slices;
    if (const char* env = std::getenv("WRNN_GEN_SLICE")) {
        if (!std::strcmp(env, "0")) slices = false;
        if (!std::strcmp(env, "1")) slices = true;
    }
    pin.gen_slices = slices && gen_frames && gen_ring_sw != 0 && persist_wide_gen_rot_usable(h->cfg.mode);
    plan_call(pin, h->rates, pout);
    const auto& lplan = pout.lplan;
    const int Bplan = pout.Bplan;
    const StreamPlan splan = plan_streams(pin, pout, h->pw.p1x4, gen_frames, gen_ring_sw);
    bool use_p = false;
    if (want != WRNN_ENGINE_CHAIN) {
        if (!h->pw.ok)
            why = "model is not fatchord (512 / 512), runtimeracer (256 / 256) or geneing (256 / 128) "
                  "with <= 1024 classes";
        else if (lplan.empty()) why = "no register-resident variant for this class count";
        else if (!splan.persist_ok)  // (plan_streams: the streams this call would write)
            why = "P1 / noise workspace for " + std::to_string(B) + " rows x " + std::to_string(S) +
                  " steps exceeds " + std::to_string((long long)(kPersistWsBytes / (1 << 30))) + " GiB";
        else if (h->persist_failed && want != WRNN_ENGINE_PERSIST)
            why = "persistent launches failed " + std::to_string(kPersistMaxStreak) +
                  " calls in a row on this handle (" + h->fallback_reason + ")";
        else if (S >= (1 << 21)) why = "seq_len >= 2^21 (step tags)";
        else if (!persist_device_ok(h)) why = "device is not a 256-CU gfx950";
        else use_p = true;
        if (want == WRNN_ENGINE_PERSIST && !use_p)
            return fail(WRNN_ERR_INVALID, "persist engine unavailable: " + why);
    }
    const int Bp = use_p ? Bplan : B;  // persistent groups carry nr rows per launch
    h->p_plan = use_p ? lplan : std::vector<PLaunch>();
    h->wrot = use_p ? pout.wrot : std::vector<WLaunch>();
    h->rot_plan = use_p ? pout.rot : RotPlan();
    // P1: the fatchord launches (register-resident and wide) form it in-kernel when the
    // per-frame form exists; the [S][B][4H] stream is written only for the other kernels
    h->p1_ring = use_p && pout.p1_ring;
    h->sparse_call = use_p && pout.sparse;
    h->sparse_wide_call = false;
    if (use_p)
        for (const auto& L : lplan) h->sparse_wide_call |= L.sp;
    // (the fatchord wide launches form P1 in-kernel too; runtimeracer and geneing: calls of wide
    // launches only -- plan_streams)
    h->p1_stream = use_p && splan.p1_stream;
    h->gen_ring = use_p && splan.gen_ring;
    h->last_p1_bytes = use_p ? splan.p1_bytes : 0.0;
    h->last_noise_bytes = use_p ? splan.noise_bytes : 0.0;
    // MelResNet frame columns: utterance u at [col0[u], col0[u] + T[u])
    std::vector<int> Ts(n_utts), col0(n_utts);
    int Tsum = 0;
    for (int u = 0; u < n_utts; ++u) {
        Ts[u] = plan[u].T;
        col0[u] = Tsum;
        Tsum += plan[u].T;
    }
    CHECK(ensure_workspace(h, Bp, S, P, Fr + 1, Tmax, Tsum));
    auto& ws = h->ws;
    h->last_B = B;
    h->last_Bp = Bp;
    h->last_S = S;
    h->last_T0 = plan[0].T;
    h->last_L0 = plan[0].L;
    // rows (pad rows repeat the last real row's addressing; their outputs are never read)
    std::vector<RowInfo> rows(Bp);
    for (int u = 0; u < n_utts; ++u) {
        const UttPlan& p = plan[u];
        for (int f = 0; f < p.B; ++f) {
            RowInfo& ri = rows[p.row0 + f];
            ri.rel0 = batched ? (p.f0 + f) * (target + overlap) : 0;
            ri.pos0 = p.pbase + ri.rel0;
            ri.L = p.L;
            ri.fbase = p.fbase;
            ri.fold = p.f0 + f;  // the global fold index keys the noise
            ri.stream = ustreams.empty() ? h->stream_ctr + (uint32_t)u : ustreams[u];
        }
        if (row_offset) row_offset[u] = p.row0;
    }
    for (int r = B; r < Bp; ++r) rows[r] = rows[B - 1];
    if (row_offset) row_offset[n_utts] = B;
    h->rows_host = rows;
    HIPC(hipMemcpyAsync(ws.rows.p, rows.data(), rows.size() * sizeof(RowInfo),
                        hipMemcpyHostToDevice, h->stream));
    CHECK(setup_debug_logits(h, S, Bp));
    // upsample + conditioning per utterance (cI folded with row stride Bp)
    if (use_p)  // (ring only: step 0 for k_persist_init)
        CHECK(h->pws.P1.alloc((size_t)(h->p1_stream ? S : 1) * Bp * (h->pw.p1x4 ? 4 : 3) * kPH * sizeof(float)));
    if (use_p) {  // noise on the side stream, concurrent with the upsample / conditioning GEMMs
        if (!h->side) {
            HIPC(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking));
            HIPC(hipEventCreateWithFlags(&h->rows_ready, hipEventDisableTiming));
            HIPC(hipEventCreateWithFlags(&h->noise_done, hipEventDisableTiming));
        }
        HIPC(hipEventRecord(h->rows_ready, h->stream));
        HIPC(hipStreamWaitEvent(h->side, h->rows_ready, 0));
        CHECK(persist_noise(h, S, h->side));
        HIPC(hipEventRecord(h->noise_done, h->side));
        h->noise_pending = true;
    }
    if (use_p && h->pw.p1x4 && h->pw.p1taps_ok && p1_frames_enabled()) {
        // per-frame P1 projections of every utterance at its frame slots; guards stay zero
        const size_t bytes = (size_t)ws.Fcap * 4 * h->H * sizeof(float);
        CHECK(ws.q4.alloc(bytes));
        CHECK(ws.a4.alloc(bytes));
        HIPC(hipMemsetAsync(ws.q4.p, 0, bytes, h->stream));
    }
    CHECK(run_resnet(h, n_utts, mels, Ts.data(), col0.data(), Tsum));
    for (int u = 0; u < n_utts; ++u)
        CHECK(run_upsample(h, mels[u], plan[u].T, plan[u].B, batched ? target + overlap : 0, S, Bp,
                           plan[u].row0, plan[u].fbase, use_p ? h->pws.P1.f() : nullptr, col0[u],
                           plan[u].f0));
    int rc = WRNN_OK;
    if (use_p) {
        rc = run_persist(h, S, cb, user);
        if (rc == kPersistFallback && want == WRNN_ENGINE_PERSIST) {
            // the caller asked for PERSIST explicitly: report, never substitute another engine
            ++h->persist_fail_streak;
            (void)hipStreamSynchronize(h->stream);
            return WRNN_ERR_HIP;  // g_err: "persistent launch: ..."
        }
        if (rc == kPersistFallback) {
            // the persistent launch could not run (e.g. CUs unavailable): same call on CHAIN,
            // counted (wrnn_fallback_info) and warned; AUTO keeps trying PERSIST on later calls
            // until kPersistMaxStreak calls in a row have failed
            ++h->fallbacks;
            h->fallback_reason = g_err;
            h->persist_failed = ++h->persist_fail_streak >= kPersistMaxStreak;
            std::fprintf(stderr, "[wavernn-mi355x] WARNING: persist engine failed (%s); this call runs on the "
                                 "chain engine (~14x slower)\n", g_err.c_str());
            use_p = false;
            h->last_p1_bytes = h->last_noise_bytes = 0.0;  // (wrnn_stream_info: 0 after a CHAIN call)
            if (h->pw.p1x4)  // cI was not written (P1 carried it): conditioning again, cI only
                for (int u = 0; u < n_utts; ++u)
                    CHECK(run_upsample(h, mels[u], plan[u].T, plan[u].B, batched ? target + overlap : 0,
                                       S, Bp, plan[u].row0, plan[u].fbase, nullptr, col0[u], plan[u].f0));
            h->last_B = Bp;  // chain runs every padded row (cI stride is Bp)
            rc = run_chain(h, S, cb, user);
            h->last_B = B;
        }
    } else {
        rc = run_chain(h, S, cb, user);
    }
    if (rc) {
        (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    h->last_engine = use_p ? WRNN_ENGINE_PERSIST : WRNN_ENGINE_CHAIN;
    if (use_p) h->persist_fail_streak = 0;
    if (seq_len) *seq_len = S;
    if (ustreams.empty()) h->stream_ctr += (uint32_t)n_utts;
    else h->stream_ctr = *std::max_element(ustreams.begin(), ustreams.end()) + 1u;
    return WRNN_OK;
}

int collect_timing(wrnn_handle* h) {
    if (h->last_engine == WRNN_ENGINE_PERSIST) {
        // one stage per launch kind: HIP-event duration of each persistent launch on its stream
        const int ns = (int)h->pstages.size();
        h->stage_avg_us.assign(ns, 0.0);
        h->stage_launches.assign(ns, 0);
        h->p_avg_steps = 0;
        if (!h->timing || h->pev.empty()) return WRNN_OK;
        HIPC(hipStreamSynchronize(h->stream));
        double steps = 0;
        const int nl = (int)h->pev.size() / 2;
        for (int i = 0; i < nl; ++i) {
            float ms = 0;
            HIPC(hipEventElapsedTime(&ms, h->pev[2 * i], h->pev[2 * i + 1]));
            for (int k = 0; k < ns; ++k)
                if (h->pstages[k].wide == h->pev_kind[i]) {
                    h->stage_avg_us[k] += ms * 1000.0;
                    h->stage_launches[k] += 1;
                }
            steps += h->pev_steps[i];
        }
        for (int k = 0; k < ns; ++k)
            if (h->stage_launches[k]) h->stage_avg_us[k] /= h->stage_launches[k];
        h->p_avg_steps = steps / nl;
        return WRNN_OK;
    }
    const int ns = (int)h->stages.size();
    h->stage_avg_us.assign(ns, 0.0);
    h->stage_launches.assign(ns, 0);
    if (!h->timing) return WRNN_OK;
    const int S = h->last_S;
    const int nt = (S - 1) / kStampEvery + 1;
    std::vector<uint32_t> st((size_t)nt * ns * kMaxStampWG * 2);
    HIPC(hipStreamSynchronize(h->stream));
    HIPC(hipMemcpy(st.data(), h->ws.stamps.p, st.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < nt; ++i) {
        const int t = i * kStampEvery;
        for (int s = 0; s < ns; ++s) {
            StageArgs a;
            int K;
            if (build_stage_args(h, s, t, S, false, &a, &K)) continue;
            const int nwg = std::min(kMaxStampWG, a.tile_start[a.nseg] * h->nrt);
            const uint32_t* p = st.data() + ((size_t)i * ns + s) * kMaxStampWG * 2;
            bool ok = true;
            long long lo = 0, hi = 0;
            const uint32_t ref = p[0];
            for (int w = 0; w < nwg && ok; ++w) {
                if (p[2 * w] == 0 && p[2 * w + 1] == 0) ok = false;
                const long long b = (int32_t)(p[2 * w] - ref), e = (int32_t)(p[2 * w + 1] - ref);
                lo = w ? std::min(lo, b) : b;
                hi = w ? std::max(hi, e) : e;
            }
            if (!ok || hi <= lo) continue;
            h->stage_avg_us[s] += (double)(hi - lo) * 0.01;  // 100 MHz ticks -> us
            h->stage_launches[s] += 1;
        }
    }
    for (int s = 0; s < ns; ++s)
        if (h->stage_launches[s]) h->stage_avg_us[s] /= h->stage_launches[s];
    return WRNN_OK;
}

}  // namespace

// =========================================================================================
// extern "C" ABI
// =========================================================================================
extern "C" {

const char* wrnn_version(void) { return "wavernn-mi355x 0.1 (gfx950)"; }

int wrnn_internal_fail(int code, const char* msg) { return fail(code, msg ? msg : ""); }

int wrnn_load_bin(wrnn_handle* h, const void* data, size_t bytes) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    auto put = [](void* u, const char* name, const float* d, const int64_t* shape, int ndim) -> int {
        return wrnn_load_tensor(static_cast<wrnn_handle*>(u), name, d, shape, ndim);
    };
    const int rc = wrnn_bin_read(data, bytes, &h->cfg, put, h);
    if (rc) return rc;
    return wrnn_finalize(h);
}

const char* wrnn_last_error(void) { return g_err.c_str(); }

int wrnn_device_count(int* count) {
    if (!count) return fail(WRNN_ERR_INVALID, "null count");
    HIPC(hipGetDeviceCount(count));
    return WRNN_OK;
}

int wrnn_create(const wrnn_config* cfg, int device, wrnn_handle** out) {
    if (!cfg || !out) return fail(WRNN_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->model_type != WRNN_MODEL_FATCHORD && cfg->model_type != WRNN_MODEL_RUNTIMERACER &&
        cfg->model_type != WRNN_MODEL_GENEING)
        return fail(WRNN_ERR_INVALID, "Invalid model type " + std::to_string(cfg->model_type));
    if (cfg->mode != WRNN_MODE_RAW && cfg->mode != WRNN_MODE_MOL && cfg->mode != WRNN_MODE_BETA)
        return fail(WRNN_ERR_INVALID, "Unknown model mode value - " + std::to_string(cfg->mode));
    if (cfg->mode == WRNN_MODE_BETA && cfg->model_type != WRNN_MODEL_GENEING)
        return fail(WRNN_ERR_INVALID, "BETA mode is the geneing 'RAW' head only");
    if (cfg->mode == WRNN_MODE_RAW && (cfg->bits < 2 || cfg->bits > 12))
        return fail(WRNN_ERR_INVALID, "bits must be in [2, 12]");
    if (cfg->n_upsample < 1 || cfg->n_upsample > 4)
        return fail(WRNN_ERR_INVALID, "n_upsample must be in [1, 4]");
    int prod = 1;
    for (int i = 0; i < cfg->n_upsample; ++i) prod *= cfg->upsample_factors[i];
    if (prod != cfg->hop_length)
        return fail(WRNN_ERR_INVALID, "prod(upsample_factors) != hop_length");  // base.py:27
    // aux split: 4 parts (fatchord, runtimeracer), 2 parts (geneing_version.py:106)
    const int n_aux = cfg->model_type == WRNN_MODEL_GENEING ? 2 : 4;
    if (cfg->res_out_dims % n_aux || cfg->res_out_dims / n_aux < 2)
        return fail(WRNN_ERR_INVALID, "res_out_dims must be a multiple of " + std::to_string(n_aux));
    std::unique_ptr<wrnn_handle> h(new wrnn_handle());
    h->cfg = *cfg;
    h->device = device;
    h->H = cfg->rnn_dims;
    h->F = cfg->fc_dims;
    h->A = cfg->res_out_dims / n_aux;
    h->C = cfg->compute_dims;
    h->R = cfg->res_out_dims;
    h->feat = cfg->feat_dims;
    h->hop = cfg->hop_length;
    h->n_classes = cfg->mode == WRNN_MODE_RAW ? (1 << cfg->bits) : cfg->mode == WRNN_MODE_BETA ? 2 : 30;
    h->n_gru = cfg->model_type == WRNN_MODEL_FATCHORD ? 2 : cfg->model_type == WRNN_MODEL_GENEING ? 1 : 4;
    h->indent = cfg->pad * prod;
    build_expected(h.get());
    h->rates = load_rates();
    HIPC(hipSetDevice(device));
    HIPC(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    *out = h.release();
    return WRNN_OK;
}

void wrnn_destroy(wrnn_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    while (!h->sessions.empty()) wrnn_stream_close(h->sessions.back());  // (stream.hip)
    delete h;
}

int wrnn_load_tensor(wrnn_handle* h, const char* name, const float* data, const int64_t* shape,
                     int ndim) {
    if (!h || !name) return fail(WRNN_ERR_INVALID, "null argument");
    auto it = h->expected.find(name);
    if (it == h->expected.end()) return WRNN_OK;  // e.g. "step", num_batches_tracked
    if (!data || !shape) return fail(WRNN_ERR_INVALID, "null data");
    const auto& ex = it->second;
    bool ok = (int)ex.size() == ndim;
    for (int i = 0; ok && i < ndim; ++i) ok = ex[i] == shape[i];
    if (!ok) {
        std::string s = "size mismatch for " + std::string(name) + ": expected (";
        for (size_t i = 0; i < ex.size(); ++i) s += std::to_string(ex[i]) + (i + 1 < ex.size() ? ", " : "");
        s += ") got (";
        for (int i = 0; i < ndim; ++i) s += std::to_string(shape[i]) + (i + 1 < ndim ? ", " : "");
        return fail(WRNN_ERR_INVALID, s + ")");
    }
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    h->host[name].assign(data, data + n);
    h->finalized = false;
    return WRNN_OK;
}

int wrnn_finalize(wrnn_handle* h) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    HIPC(hipSetDevice(h->device));
    return do_finalize(h);
}

int wrnn_set_seed(wrnn_handle* h, uint64_t seed) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    h->seed = seed;
    h->stream_ctr = 0;
    return WRNN_OK;
}

int wrnn_set_stream(wrnn_handle* h, uint32_t stream) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    h->stream_ctr = stream;
    return WRNN_OK;
}

int wrnn_get_stream(wrnn_handle* h, uint32_t* stream) {
    if (!h || !stream) return fail(WRNN_ERR_INVALID, "null argument");
    *stream = h->stream_ctr;
    return WRNN_OK;
}

int wrnn_set_utt_streams(wrnn_handle* h, const uint32_t* streams, int n) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    if (n < 0 || (n > 0 && !streams)) return fail(WRNN_ERR_INVALID, "bad stream list");
    h->utt_streams.assign(streams, streams + n);
    return WRNN_OK;
}

int wrnn_set_fold_ranges(wrnn_handle* h, const int* lo, const int* hi, int n) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    if (n < 0 || (n > 0 && (!lo || !hi))) return fail(WRNN_ERR_INVALID, "bad fold range list");
    h->fold_lo.assign(lo, lo + n);
    h->fold_hi.assign(hi, hi + n);
    return WRNN_OK;
}

int wrnn_fold_shape(int n_frames, int hop_length, int batched, int target, int overlap,
                    int* num_folds, int* seq_len) {
    if (!num_folds || !seq_len) return fail(WRNN_ERR_INVALID, "null argument");
    if (n_frames <= 0 || hop_length <= 0) return fail(WRNN_ERR_INVALID, "bad length");
    if (batched && (target <= 0 || overlap < 0)) return fail(WRNN_ERR_INVALID, "bad target/overlap");
    fold_shape(n_frames * hop_length, batched, target, overlap, num_folds, seq_len);
    return WRNN_OK;
}

// The one-call options (wrnn_set_utt_streams, wrnn_set_fold_ranges) belong to the next
// generate call whatever its outcome, also when it fails before generate_impl takes them.
struct DisarmOnExit {
    wrnn_handle* h;
    ~DisarmOnExit() {
        if (!h) return;
        h->utt_streams.clear();
        h->fold_lo.clear();
        h->fold_hi.clear();
    }
};

int wrnn_generate(wrnn_handle* h, const float* mel, int n_frames, int batched, int target,
                  int overlap, int16_t* labels, float* samples, size_t capacity, int* num_folds,
                  int* seq_len, wrnn_progress_fn cb, void* user) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    DisarmOnExit disarm{h};
    if (!h->finalized)
        return fail(WRNN_ERR_NOT_LOADED, "Model hasn't been loaded. Call loadWeights first.");
    if (!mel || n_frames <= 0) return fail(WRNN_ERR_INVALID, "empty mel");
    if (labels && h->cfg.mode != WRNN_MODE_RAW) return fail(WRNN_ERR_INVALID, "labels require RAW mode");
    if (!h->fold_lo.empty()) {
        h->fold_lo.clear();
        h->fold_hi.clear();
        return fail(WRNN_ERR_INVALID, "fold ranges apply to wrnn_generate_batch_device only");
    }
    HIPC(hipSetDevice(h->device));
    int B, S;
    fold_shape(n_frames * h->hop, batched, target, overlap, &B, &S);
    if (B <= 0) return fail(WRNN_ERR_INVALID, "mel too short for target/overlap");
    if ((labels || samples) && capacity < (size_t)B * S)
        return fail(WRNN_ERR_CAPACITY, "output capacity " + std::to_string(capacity) + " < " +
                                           std::to_string((size_t)B * S));
    auto& ws = h->ws;
    const size_t mbytes = (size_t)h->feat * n_frames * sizeof(float);
    if (mbytes > ws.mel_in.bytes) {
        ws.mel_in.release();
        CHECK(ws.mel_in.alloc(mbytes));
    }
    HIPC(hipMemcpyAsync(ws.mel_in.p, mel, mbytes, hipMemcpyHostToDevice, h->stream));
    const float* mels[1] = {ws.mel_in.f()};
    int roff[2];
    int S2 = 0;
    CHECK(generate_impl(h, 1, mels, &n_frames, batched, target, overlap, roff, &S2, cb, user));
    // copy rows out (device row stride = ws.S)
    if (labels)
        HIPC(hipMemcpy2DAsync(labels, S * sizeof(int16_t), ws.labels.p, ws.S * sizeof(int16_t),
                              S * sizeof(int16_t), B, hipMemcpyDeviceToHost, h->stream));
    if (samples)
        HIPC(hipMemcpy2DAsync(samples, S * sizeof(float), ws.samples.p, ws.S * sizeof(float),
                              S * sizeof(float), B, hipMemcpyDeviceToHost, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    CHECK(collect_timing(h));
    if (num_folds) *num_folds = B;
    if (seq_len) *seq_len = S;
    return WRNN_OK;
}

int wrnn_generate_batch_device(wrnn_handle* h, int n_utts, const float* const* mels,
                               const int* n_frames, int batched, int target, int overlap,
                               int16_t* labels_dev, float* samples_dev, size_t capacity,
                               int* row_offset, int* seq_len, wrnn_progress_fn cb, void* user) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    DisarmOnExit disarm{h};
    if (!mels || !n_frames || !row_offset) return fail(WRNN_ERR_INVALID, "null argument");
    if (labels_dev && h->cfg.mode != WRNN_MODE_RAW)
        return fail(WRNN_ERR_INVALID, "labels require RAW mode");
    HIPC(hipSetDevice(h->device));
    int B = 0, S = 0;
    const bool ranged = !h->fold_lo.empty() && (int)h->fold_lo.size() == n_utts;
    for (int u = 0; u < n_utts; ++u) {
        int b, s;
        if (n_frames[u] <= 0) return fail(WRNN_ERR_INVALID, "empty mel");
        fold_shape(n_frames[u] * h->hop, batched, target, overlap, &b, &s);
        if (ranged) b = std::max(0, std::min(h->fold_hi[u], b) - std::max(h->fold_lo[u], 0));
        B += b;
        S = s;
    }
    if ((labels_dev || samples_dev) && capacity < (size_t)B * S)
        return fail(WRNN_ERR_CAPACITY, "output capacity too small");
    int S2 = 0;
    CHECK(generate_impl(h, n_utts, mels, n_frames, batched, target, overlap, row_offset, &S2, cb, user));
    auto& ws = h->ws;
    if (labels_dev)
        HIPC(hipMemcpy2DAsync(labels_dev, S * sizeof(int16_t), ws.labels.p, ws.S * sizeof(int16_t),
                              S * sizeof(int16_t), B, hipMemcpyDeviceToDevice, h->stream));
    if (samples_dev)
        HIPC(hipMemcpy2DAsync(samples_dev, S * sizeof(float), ws.samples.p, ws.S * sizeof(float),
                              S * sizeof(float), B, hipMemcpyDeviceToDevice, h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    CHECK(collect_timing(h));
    if (seq_len) *seq_len = S;
    return WRNN_OK;
}

int wrnn_enable_stage_timing(wrnn_handle* h, int enable) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    h->timing = enable != 0;
    return WRNN_OK;
}

int wrnn_stage_timing(wrnn_handle* h, int stage, double* avg_us, int* launches) {
    if (!h || !avg_us || !launches) return fail(WRNN_ERR_INVALID, "null argument");
    if (stage < 0 || stage >= (int)h->stage_avg_us.size())
        return fail(WRNN_ERR_INVALID, "no timing for stage " + std::to_string(stage));
    *avg_us = h->stage_avg_us[stage];
    *launches = h->stage_launches[stage];
    return WRNN_OK;
}

int wrnn_set_gen_wide_rows(wrnn_handle* h, int rows) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    if (rows != kPWideRows && rows != kPWideGen32Rows)
        return fail(WRNN_ERR_INVALID, "rows per group of a wide launch must be 16 or 32");
    if (rows == kPWideGen32Rows && h->cfg.model_type != WRNN_MODEL_GENEING)
        return fail(WRNN_ERR_INVALID, "32-row wide launches exist for the geneing topology only");
    h->gen_wide_rows = rows;
    return WRNN_OK;
}

int wrnn_set_gen_wide_slices(wrnn_handle* h, int on) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    if (on != 0 && on != 1) return fail(WRNN_ERR_INVALID, "time-sliced wide launches: 0 (off) or 1 (on)");
    if (on && h->cfg.model_type != WRNN_MODEL_GENEING)
        return fail(WRNN_ERR_INVALID, "the time-sliced wide launches are opt-in for the geneing topology only");
    h->gen_wide_slices = on != 0;
    return WRNN_OK;
}

int wrnn_set_engine(wrnn_handle* h, int engine) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    if (engine != WRNN_ENGINE_AUTO && engine != WRNN_ENGINE_CHAIN && engine != WRNN_ENGINE_PERSIST)
        return fail(WRNN_ERR_INVALID, "unknown engine " + std::to_string(engine));
    h->engine = engine;
    return WRNN_OK;
}

int wrnn_last_engine(wrnn_handle* h, int* engine) {
    if (!h || !engine) return fail(WRNN_ERR_INVALID, "null argument");
    *engine = h->last_engine;
    return WRNN_OK;
}

int wrnn_plan_info(wrnn_handle* h, int* n_launches, int* first_row, int* rows_per_group, int* wide,
                   int cap) {
    if (!h || !n_launches) return fail(WRNN_ERR_INVALID, "null argument");
    const bool p = h->last_engine == WRNN_ENGINE_PERSIST;
    const int n = p ? (int)h->p_plan.size() : 0;
    *n_launches = n;
    for (int i = 0; i < n && i < cap; ++i) {
        if (first_row) first_row[i] = h->p_plan[i].rb;
        if (rows_per_group) rows_per_group[i] = h->p_plan[i].nr;
        if (wide) wide[i] = h->p_plan[i].wide ? 1 : 0;
    }
    return WRNN_OK;
}

int wrnn_sparse_info(wrnn_handle* h, int* available, int* last_call, double* density, int* fill_f4) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    if (available) *available = h->pw.sp_ok ? 1 : 0;
    if (last_call) *last_call = h->last_engine == WRNN_ENGINE_PERSIST && h->sparse_call ? 1 : 0;
    if (density) *density = h->pw.sp_density;
    if (fill_f4) *fill_f4 = h->pw.sp_fill;
    return WRNN_OK;
}

int wrnn_sparse_wide_info(wrnn_handle* h, int* available, int* last_call, double* density, int* fill_f4) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    if (available) *available = h->pw.wsp_img ? 1 : 0;
    if (last_call) *last_call = h->last_engine == WRNN_ENGINE_PERSIST && h->sparse_wide_call ? 1 : 0;
    if (density) *density = h->pw.wsp_density;
    if (fill_f4) *fill_f4 = h->pw.wsp_fill;
    return WRNN_OK;
}

int wrnn_fallback_info(wrnn_handle* h, int* count, char* reason, size_t reason_cap) {
    if (!h || !count) return fail(WRNN_ERR_INVALID, "null argument");
    *count = h->fallbacks;
    if (reason && reason_cap) {
        const size_t n = std::min(reason_cap - 1, h->fallback_reason.size());
        std::memcpy(reason, h->fallback_reason.data(), n);
        reason[n] = 0;
    }
    return WRNN_OK;
}

int wrnn_stage_info(wrnn_handle* h, int stage, char* name, size_t name_cap, double* bytes,
                    double* flops, int* n_stages) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    if (h->last_engine == WRNN_ENGINE_PERSIST) {
        const int ns = (int)h->pstages.size();
        if (n_stages) *n_stages = ns;
        if (stage < 0 || stage >= ns) return fail(WRNN_ERR_INVALID, "bad stage index");
        const auto& q = h->pstages[stage];
        if (name && name_cap) std::snprintf(name, name_cap, "%s", q.name.c_str());
        // per launch = steps x (recurrent weights once per step + the launch's real rows x
        // per-row-step stream) / FLOPs
        // (summed over the kind's launches, per launch: launches of different steps and rows --
        // the time-sliced wide plan -- are counted each with its own)
        const double nl = q.launches ? q.launches : 1.0;
        if (bytes) *bytes = (q.steps * h->p_wbytes + q.row_steps * h->p_row_bytes) / nl;
        if (flops) *flops = q.row_steps * 2.0 * h->p_macs / nl;
        return WRNN_OK;
    }
    if (n_stages) *n_stages = (int)h->stages.size();
    if (stage < 0 || stage >= (int)h->stages.size())
        return fail(WRNN_ERR_INVALID, "bad stage index");
    const StageDesc& sd = h->stages[stage];
    if (name && name_cap) {
        std::snprintf(name, name_cap, "%s", sd.name.c_str());
    }
    const double B = h->last_B;
    double by = 0, fl = 0;
    for (const SegDesc& d : sd.segs) {
        const double n = d.w.n_out, K = d.w.K;
        by += n * K * 4.0;             // weights
        by += B * K * 4.0;             // input rows
        by += B * n * 4.0;             // outputs / gate pre-activations consumed
        if (d.kind == EPI_GRU) by += B * (3 * h->H + 3 * h->H + 2 * h->H) * 4.0;  // cond,gh,h,xout
        else by += B * n * 4.0;        // cond / bias read
        fl += 2.0 * n * K * B;
    }
    if (bytes) *bytes = by;
    if (flops) *flops = fl;
    return WRNN_OK;
}

int wrnn_debug_wide_layout(int rows_per_group) {
    const int bad = wide_layout_check(rows_per_group), bad_rr = wide_rr_layout_check(rows_per_group);
    if (bad < 0 || bad_rr < 0) return fail(WRNN_ERR_INVALID, "rows_per_group must be 1..16");
    return bad + bad_rr;
}

int wrnn_debug_wide_gen_layout(int rows_per_group) {
    const int bad = wide_gen_layout_check(rows_per_group);
    if (bad < 0) return fail(WRNN_ERR_INVALID, "rows_per_group must be 1..16");
    return bad;
}

int wrnn_debug_wide_gen_mol_layout(int rows_per_group, int n_logits) {
    const int bad = wide_gen_mol_layout_check(rows_per_group, n_logits);
    if (bad < 0) return fail(WRNN_ERR_INVALID, "rows_per_group must be 1..16 and n_logits 30 (MOL) or 2 (Beta)");
    return bad;
}

int wrnn_debug_wide_gen32_layout(int rows_per_group) {
    const int bad = wide_gen32_layout_check(rows_per_group);
    if (bad < 0) return fail(WRNN_ERR_INVALID, "rows_per_group must be 1..32");
    return bad;
}

int wrnn_debug_wide_gen32_mol_layout(int rows_per_group, int n_logits) {
    const int bad = wide_gen32_mol_layout_check(rows_per_group, n_logits);
    if (bad < 0) return fail(WRNN_ERR_INVALID, "rows_per_group must be 1..32 and n_logits 30 (MOL) or 2 (Beta)");
    return bad;
}

int wrnn_debug_wide_mol_layout(int rows_per_group) {
    const int bad = wide_mol_layout_check(rows_per_group);
    if (bad < 0) return fail(WRNN_ERR_INVALID, "rows_per_group must be 1..16");
    return bad;
}

int wrnn_debug_wide_rr_mol_layout(int rows_per_group) {
    const int bad = wide_rr_mol_layout_check(rows_per_group);
    if (bad < 0) return fail(WRNN_ERR_INVALID, "rows_per_group must be 1..16");
    return bad;
}

int wrnn_debug_beta(uint64_t seed, uint32_t stream, uint32_t step, uint32_t row, float alpha,
                    float beta, float* out) {
    if (!out) return fail(WRNN_ERR_INVALID, "null argument");
    if (!(alpha > 0.f) || !(beta > 0.f)) return fail(WRNN_ERR_INVALID, "alpha, beta must be > 0");
    *out = beta_sample(alpha, beta, step, row, stream, (uint32_t)(seed & 0xffffffffu),
                       (uint32_t)(seed >> 32));
    return WRNN_OK;
}

int wrnn_set_rates(wrnn_handle* h, const char* table) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    if (!table) {
        h->rates = load_rates();
        return WRNN_OK;
    }
    PlanRates R;
    std::string err;
    if (!parse_rates(table, R, err)) return fail(WRNN_ERR_INVALID, "rate table: " + err);
    R.source = "wrnn_set_rates";
    h->rates = R;
    return WRNN_OK;
}

int wrnn_get_rates(wrnn_handle* h, char* buf, size_t cap) {
    if (!h || !buf || cap == 0) return fail(WRNN_ERR_INVALID, "null argument");
    const std::string t = rates_text(h->rates);
    if (t.size() + 1 > cap) return fail(WRNN_ERR_CAPACITY, "rate table needs " + std::to_string(t.size() + 1) + " bytes");
    std::memcpy(buf, t.c_str(), t.size() + 1);
    return WRNN_OK;
}

int wrnn_stream_info(wrnn_handle* h, uint64_t* p1_bytes, uint64_t* noise_bytes) {
    if (!h || !p1_bytes || !noise_bytes) return fail(WRNN_ERR_INVALID, "null argument");
    *p1_bytes = (uint64_t)h->last_p1_bytes;
    *noise_bytes = (uint64_t)h->last_noise_bytes;
    return WRNN_OK;
}

int wrnn_persist_steps(wrnn_handle* h, int stage, double* steps_per_launch) {
    if (!h || !steps_per_launch) return fail(WRNN_ERR_INVALID, "null argument");
    if (h->last_engine != WRNN_ENGINE_PERSIST || stage < 0 || stage >= (int)h->pstages.size())
        return fail(WRNN_ERR_INVALID, "bad stage index");
    const auto& q = h->pstages[stage];
    *steps_per_launch = q.launches ? q.steps / q.launches : 0.0;
    return WRNN_OK;
}

int wrnn_rot_info(wrnn_handle* h, int* launches, int* n_hi, int* n_lo) {
    if (!h || !launches || !n_hi || !n_lo) return fail(WRNN_ERR_INVALID, "null argument");
    const bool rot = !h->p_plan.empty() && h->p_plan[0].rot >= 0 && !h->p_plan[0].wide &&
                     h->last_engine == WRNN_ENGINE_PERSIST;
    *launches = rot ? h->rot_plan.K : 0;
    *n_hi = rot ? h->rot_plan.n_hi : 0;
    *n_lo = rot ? h->rot_plan.n_lo : 0;
    return WRNN_OK;
}

int wrnn_debug_decide(uint64_t seed, uint32_t stream, uint32_t step, uint32_t fold, const float* logits,
                      int n_classes, int* label, double* margin) {
    if (!logits || !label) return fail(WRNN_ERR_INVALID, "null argument");
    if (n_classes < 2 || n_classes > 4096) return fail(WRNN_ERR_INVALID, "n_classes must be in [2, 4096]");
    const uint32_t k0 = (uint32_t)(seed & 0xffffffffu), k1 = (uint32_t)(seed >> 32);
    CandKey best{0u, 0u};
    double v1 = -INFINITY, v2 = -INFINITY;
    for (int k = 0; k < n_classes; ++k) {
        const U4 o = philox4x32_10((uint32_t)(k >> 2), step, fold, stream, k0, k1);
        const uint32_t w = (k & 3) == 0 ? o.x : (k & 3) == 1 ? o.y : (k & 3) == 2 ? o.z : o.w;
        const uint32_t gq = gumbel_q_of(w);
        const CandKey c = cand_key(logits[k], gq, k);
        if (c.hi > best.hi || (c.hi == best.hi && c.lo > best.lo)) best = c;
        const double v = (double)logits[k] + ((double)gq * (1.0 / kGumbelScale) - kGumbelOffset);
        if (v > v1) {
            v2 = v1;
            v1 = v;
        } else if (v > v2) {
            v2 = v;
        }
    }
    *label = key_cls(best.lo);
    if (margin) *margin = v1 - v2;
    return WRNN_OK;
}

int wrnn_debug_noise(wrnn_handle* h, int n_steps, float* out, size_t capacity) {
    // the sampler draws its noise in-kernel from philox.h; this regenerates the same stream
    // for the last call's rows with the same device code into a scratch buffer
    if (!h || !out) return fail(WRNN_ERR_INVALID, "null argument");
    if (h->cfg.mode != WRNN_MODE_RAW) return fail(WRNN_ERR_INVALID, "RAW mode only");
    const size_t n = (size_t)n_steps * h->last_B * h->n_classes;
    if (n_steps > h->last_S || capacity < n) return fail(WRNN_ERR_CAPACITY, "capacity");
    CHECK(h->ws.noise.alloc(n * sizeof(float)));
    HIPC(launch_noise_raw(h->ws.noise.f(), n_steps, h->last_B, h->n_classes,
                          (const RowInfo*)h->ws.rows.p, (uint32_t)(h->seed & 0xffffffffu),
                          (uint32_t)(h->seed >> 32), h->stream));
    HIPC(hipStreamSynchronize(h->stream));
    HIPC(hipMemcpy(out, h->ws.noise.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return WRNN_OK;
}

int wrnn_debug_upsample(wrnn_handle* h, float* mel_out, size_t mel_cap, float* aux_out,
                        size_t aux_cap) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    HIPC(hipStreamSynchronize(h->stream));
    const size_t nm = (size_t)h->feat * h->last_L0, na = (size_t)h->R * h->last_T0;
    if (mel_out) {
        if (mel_cap < nm) return fail(WRNN_ERR_CAPACITY, "mel capacity");
        if (!h->melup_valid)
            return fail(WRNN_ERR_INVALID, "the last call did not materialise the upsampled mel "
                                          "(persistent engine, per-frame P1): see wrnn_debug_p1");
        HIPC(hipMemcpy(mel_out, h->ws.melup.p, nm * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (aux_out) {
        if (aux_cap < na) return fail(WRNN_ERR_CAPACITY, "aux capacity");
        // utterance 0's columns [0, T0) of the call's [R][N] MelResNet output
        HIPC(hipMemcpy2D(aux_out, (size_t)h->last_T0 * sizeof(float), h->ws.Rb.p, (size_t)h->ws.N * sizeof(float),
                         (size_t)h->last_T0 * sizeof(float), h->R, hipMemcpyDeviceToHost));
    }
    return WRNN_OK;
}

int wrnn_set_debug_steps(wrnn_handle* h, const int* steps, int n) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    if (n < 0 || n > kDbgSteps || (n > 0 && !steps))
        return fail(WRNN_ERR_INVALID, "at most " + std::to_string(kDbgSteps) + " debug steps");
    for (int i = 0; i < n; ++i)
        if (steps[i] < 0) return fail(WRNN_ERR_INVALID, "negative debug step");
    h->dbg_steps.assign(steps, steps + n);
    return WRNN_OK;
}

int wrnn_debug_logits(wrnn_handle* h, int step, int row, float* out, size_t capacity) {
    if (!h || !out) return fail(WRNN_ERR_INVALID, "null argument");
    HIPC(hipStreamSynchronize(h->stream));
    if (!h->dbg.out) return fail(WRNN_ERR_INVALID, "the last call recorded no logits (wrnn_set_debug_steps)");
    int k = -1;
    for (size_t i = 0; i < h->dbg_steps.size(); ++i)
        if (h->dbg_steps[i] == step) k = (int)i;
    if (k < 0 || step >= h->dbg_S) return fail(WRNN_ERR_INVALID, "step " + std::to_string(step) + " was not recorded");
    if (row < 0 || row >= h->last_B) return fail(WRNN_ERR_INVALID, "row out of range");
    const int n = h->n_classes;
    if (capacity < (size_t)n) return fail(WRNN_ERR_CAPACITY, "logit capacity");
    HIPC(hipMemcpy(out, h->dbg.out + ((size_t)k * h->dbg_rows + row) * n, n * sizeof(float),
                   hipMemcpyDeviceToHost));
    return WRNN_OK;
}

int wrnn_debug_p1(wrnn_handle* h, int step, int row, float* out, size_t capacity) {
    if (!h || !out) return fail(WRNN_ERR_INVALID, "null argument");
    HIPC(hipStreamSynchronize(h->stream));
    if (h->last_engine != WRNN_ENGINE_PERSIST || !h->pw.p1x4 || !h->pws.P1.p)
        return fail(WRNN_ERR_INVALID, "the last call did not run the persistent engine");
    const int np = 4 * h->H, Bp = h->last_Bp;
    if (step < 0 || step >= h->last_S || row < 0 || row >= Bp)
        return fail(WRNN_ERR_INVALID, "step / row out of range");
    if (capacity < (size_t)np) return fail(WRNN_ERR_CAPACITY, "P1 capacity");
    if (h->p1_stream || step == 0) {
        HIPC(hipMemcpy(out, h->pws.P1.f() + ((size_t)step * Bp + row) * np, np * sizeof(float),
                       hipMemcpyDeviceToHost));
        return WRNN_OK;
    }
    // ring: the launch formed this step's P1 in-kernel; form it here from the same device
    // tables with the same fp32 operations (k_persist p1_store / k_p1_expand)
    const RowInfo ri = h->rows_host[row];
    const int hop = h->hop, p = ri.rel0 + step, nfr = ri.L / hop;
    const bool in = p < ri.L;
    const int f = in ? p / hop : 0, s = in ? p - f * hop : 0;
    std::vector<float> taps(8), q((size_t)np), a((size_t)np);
    HIPC(hipMemcpy(taps.data(), h->pw.p1taps + (size_t)s * 8, 8 * sizeof(float), hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(a.data(), h->ws.a4.f() + (size_t)(in ? ri.fbase + 1 + f : ri.fbase) * np,
                   np * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<float> m((size_t)np, 0.f);
    for (int k = 0; k < 5; ++k) {
        const int j = f - 2 + k;
        const int slot = in && j >= 0 && j < nfr ? ri.fbase + 1 + j : ri.fbase;
        HIPC(hipMemcpy(q.data(), h->ws.q4.f() + (size_t)slot * np, np * sizeof(float),
                       hipMemcpyDeviceToHost));
        for (int c = 0; c < np; ++c) m[c] = std::fma(taps[k], q[c], m[c]);
    }
    for (int c = 0; c < np; ++c) {
        volatile float v = m[c] + a[c];
        out[c] = v;
    }
    return WRNN_OK;
}

}  // extern "C"

// The streaming sessions (wrnn_stream_*): a file of their own, compiled as part of this
// translation unit because they work on the handle defined above.
#include "stream.hip"
