// Streaming vocoder sessions (include/wavernn_mi355x.h wrnn_stream_*): mel frames
// in as they arrive, labels out as soon as their conditioning is final. No reference equivalent;
// a streamed utterance equals wrnn_generate(batched = 0) on the same mel, seed and stream bit for
// bit. Included at the end of runtime.hip (the sessions work on its wrnn_handle).
//
// A session owns its device memory: the mel (zero-padded by `pad` columns at either end, as
// conv_in's im2col pads it), the per-frame tables p1q / p1a / fcond laid out as generate_impl lays
// them ([guard][zero frame = fbase = 1][frames][guard][guard]), the chunk state of its one row, a
// noise window and the outputs of one launch. Per push the rows that became final are computed
// with the one-shot path's k_gemm on column windows (k_gemm sums every output element over k in
// one order whatever N or the column's place in its tile), per advance one
// streaming launch of k_persist runs every ready step of up to 8 sessions.
#include <limits>

#include "stream_host.h"

namespace {

// frames past a step's own whose projections the P1 taps read (k_p1_expand: f - 2 .. f + 2; the
// in-kernel ring reads f - 2 + k0 .. f + 1 + k0, k0 <= 1)
constexpr int kP1TapReach = 2;
constexpr int kStreamFbase = 1;
constexpr uint32_t kNaNWord = 0x7fc00000u;

int fill_words(void* p, uint32_t word, size_t n, hipStream_t st) {
    HIPC(hipMemsetD32Async((hipDeviceptr_t)p, (int)word, n, st));
    return WRNN_OK;
}

}  // namespace

struct wrnn_stream {
    wrnn_handle* h = nullptr;
    int max_frames = 0, frames = 0, aux_done = 0, la = 0, mel_ld = 0;
    bool ended = false;
    int64_t steps_done = 0;
    uint64_t seed = 0;
    uint32_t stream = 0;
    DevBuf mel, act0, act1, Rb, q4, a4, fcond, st, P1, gumbel, labels, samples;

    int64_t ready() const { return stream_ready_steps(frames, ended, h->hop, la); }
    size_t slots() const { return (size_t)max_frames + 4; }
};

namespace {

// the zero-frame slot of the three tables, by the GEMMs that write it in the one-shot call (row 0
// of a frame-A product: bias only)
int stream_zero_frame(wrnn_stream* s) {
    wrnn_handle* h = s->h;
    const int np = 4 * h->H;
    GemmA a{};
    GemmB b{};
    GemmEp e{};
    a.kind = 2;
    a.R = s->mel.f();
    a.ldr = s->mel_ld;
    b.kind = 0;
    b.p = h->pw.M1T;
    b.ld = np;
    e.kind = 0;
    e.D = s->q4.f() + (size_t)kStreamFbase * np;
    e.ld = np;
    e.bias = h->pw.zero_np;
    HIPC(launch_gemm(1, np, h->feat, a, b, e, h->stream));
    b.p = h->pw.M1T + (size_t)h->feat * np;
    e.D = s->a4.f() + (size_t)kStreamFbase * np;
    e.bias = h->pw.bP1;
    HIPC(launch_gemm(1, np, h->A - 1, a, b, e, h->stream));
    for (const auto& ac : h->auxc) {
        GemmB b5{};
        GemmEp e5{};
        a.r_off = ac.slice * h->A;
        b5.kind = 0;
        b5.p = ac.WT;
        b5.ld = ac.n_out;
        e5.kind = 0;
        e5.D = s->fcond.f() + (size_t)kStreamFbase * h->cond_width + ac.offset;
        e5.ld = h->cond_width;
        e5.bias = ac.bias;
        HIPC(launch_gemm(1, ac.n_out, h->A, a, b5, e5, h->stream));
    }
    return WRNN_OK;
}

// p1q rows of frames [f0, f1): M1_mel mel(frame) -- final as soon as the frame is there
int stream_q_rows(wrnn_stream* s, int f0, int f1) {
    wrnn_handle* h = s->h;
    const int np = 4 * h->H, n = f1 - f0;
    if (n <= 0) return WRNN_OK;
    GemmA a{};
    GemmB b{};
    GemmEp e{};
    a.kind = 3;  // row m = frame f0 + m
    a.R = s->mel.f() + h->cfg.pad + f0;
    a.ldr = s->mel_ld;
    b.kind = 0;
    b.p = h->pw.M1T;
    b.ld = np;
    e.kind = 0;
    e.D = s->q4.f() + (size_t)(kStreamFbase + 1 + f0) * np;
    e.ld = np;
    e.bias = h->pw.zero_np;
    HIPC(launch_gemm(n, np, h->feat, a, b, e, h->stream));
    return WRNN_OK;
}

// MelResNet columns of frames [f0, f1) (run_resnet on a column window: conv_in reads mel frames
// f - pad .. f + pad, zeros outside the utterance; the other layers are per column), then their
// p1a and fcond rows (run_upsample's frame-A products on the window)
int stream_aux_rows(wrnn_stream* s, int f0, int f1) {
    wrnn_handle* h = s->h;
    hipStream_t st = h->stream;
    const int n = f1 - f0, C = h->C, R = h->R, np = 4 * h->H;
    if (n <= 0) return WRNN_OK;
    const int ksz = 2 * h->cfg.pad + 1;
    {
        GemmA a{};
        GemmB b{};
        GemmEp e{};
        a.kind = 0;
        a.p = h->Wci;
        a.ld = h->feat * ksz;
        // im2col over the session's padded mel: column f0 + i of the buffer is frame f0 + i - pad,
        // so out frame f0 + j reads columns j + kk of the window base (the pad columns hold the
        // zeros the one-shot im2col substitutes)
        b.kind = 1;
        b.p = s->mel.f() + f0;
        b.T = s->mel_ld;
        b.pad = 0;
        b.ksz = ksz;
        e.kind = 2;
        e.D = s->act0.f();
        e.ld = n;
        e.alpha = h->bn_a;
        e.beta = h->bn_b;
        e.relu = 1;
        HIPC(launch_gemm(C, n, h->feat * ksz, a, b, e, st));
    }
    for (int i = 0; i < h->cfg.res_blocks; ++i) {
        GemmA a1{};
        GemmB b1{};
        GemmEp e1{};
        a1.kind = 0;
        a1.p = h->Wres[2 * i];
        a1.ld = C;
        b1.kind = 0;
        b1.p = s->act0.f();
        b1.ld = n;
        e1.kind = 2;
        e1.D = s->act1.f();
        e1.ld = n;
        e1.alpha = h->bn_a + (size_t)(1 + 2 * i) * C;
        e1.beta = h->bn_b + (size_t)(1 + 2 * i) * C;
        e1.relu = 1;
        HIPC(launch_gemm(C, n, C, a1, b1, e1, st));
        GemmA a2 = a1;
        GemmB b2 = b1;
        GemmEp e2{};
        a2.p = h->Wres[2 * i + 1];
        b2.p = s->act1.f();
        e2.kind = 2;
        e2.D = s->act0.f();
        e2.ld = n;
        e2.alpha = h->bn_a + (size_t)(2 + 2 * i) * C;
        e2.beta = h->bn_b + (size_t)(2 + 2 * i) * C;
        e2.relu = 0;
        e2.res = s->act0.f();
        HIPC(launch_gemm(C, n, C, a2, b2, e2, st));
    }
    {
        GemmA a3{};
        GemmB b3{};
        GemmEp e3{};
        a3.kind = 0;
        a3.p = h->Wco;
        a3.ld = C;
        b3.kind = 0;
        b3.p = s->act0.f();
        b3.ld = n;
        e3.kind = 1;
        e3.D = s->Rb.f();
        e3.ld = n;
        e3.bias = h->bco;
        HIPC(launch_gemm(R, n, C, a3, b3, e3, st));
    }
    GemmA aq{};
    GemmB bq{};
    GemmEp eq{};
    aq.kind = 3;
    aq.R = s->Rb.f();
    aq.ldr = n;
    aq.r_off = 0;
    bq.kind = 0;
    bq.p = h->pw.M1T + (size_t)h->feat * np;
    bq.ld = np;
    eq.kind = 0;
    eq.D = s->a4.f() + (size_t)(kStreamFbase + 1 + f0) * np;
    eq.ld = np;
    eq.bias = h->pw.bP1;
    HIPC(launch_gemm(n, np, h->A - 1, aq, bq, eq, st));
    for (const auto& ac : h->auxc) {
        GemmA a5 = aq;
        GemmB b5{};
        GemmEp e5{};
        a5.r_off = ac.slice * h->A;
        b5.kind = 0;
        b5.p = ac.WT;
        b5.ld = ac.n_out;
        e5.kind = 0;
        e5.D = s->fcond.f() + (size_t)(kStreamFbase + 1 + f0) * h->cond_width + ac.offset;
        e5.ld = h->cond_width;
        e5.bias = ac.bias;
        HIPC(launch_gemm(n, ac.n_out, h->A, a5, b5, e5, st));
    }
    return WRNN_OK;
}

// why a handle cannot stream ("" when it can)
std::string stream_refusal(wrnn_handle* h) {
    if (!h->finalized) return "the model is not loaded";
    if (h->cfg.model_type != WRNN_MODEL_FATCHORD || !h->pw.ok || h->pw.rr || h->pw.gen || h->H != kPH)
        return "streaming sessions need a fatchord model (rnn_dims = fc_dims = 512, <= 1024 classes)";
    if (h->cfg.mode != WRNN_MODE_RAW) return "streaming sessions need the RAW head";
    int want = h->engine;
    if (const char* env = std::getenv("WRNN_ENGINE")) {
        if (!std::strcmp(env, "chain")) want = WRNN_ENGINE_CHAIN;
        else if (!std::strcmp(env, "persist")) want = WRNN_ENGINE_PERSIST;
        else if (!std::strcmp(env, "auto")) want = WRNN_ENGINE_AUTO;
    }
    if (want == WRNN_ENGINE_CHAIN) return "streaming sessions run on the persistent engine; this handle is set to CHAIN";
    if (!p1_ring_ok(h)) return "the model has no per-frame P1 form (the upsampler's taps do not fit 4 frames)";
    if (!persist_device_ok(h)) return "device is not a 256-CU gfx950";
    const int sc = persist_stream_scratch(h->pw.cpw);
    if (sc != 0) return "the streaming kernel instance for this class count is not spill-free (" + std::to_string(sc) + " bytes of scratch)";
    return "";
}

}  // namespace

extern "C" {

int wrnn_stream_open(wrnn_handle* h, int max_frames, wrnn_stream** out) {
    if (!h || !out) return fail(WRNN_ERR_INVALID, "null argument");
    *out = nullptr;
    if (max_frames < 1) return fail(WRNN_ERR_INVALID, "max_frames must be positive");
    HIPC(hipSetDevice(h->device));
    const std::string why = stream_refusal(h);
    if (!why.empty()) return fail(WRNN_ERR_INVALID, "wrnn_stream_open: " + why);
    const int np = 4 * h->H, pad = h->cfg.pad, cw = h->cond_width;
    // the kernel addresses a table through one buffer resource (32-bit offsets below 2 GiB); the
    // step count keeps its 21-bit exchange tags per launch
    if ((double)(max_frames + 4) * std::max(np, cw) * sizeof(float) >= 2147483648.0 ||
        (double)max_frames * h->hop >= (double)(1 << 21))
        return fail(WRNN_ERR_INVALID, "max_frames too large for one session");
    std::unique_ptr<wrnn_stream> s(new wrnn_stream());
    s->h = h;
    s->max_frames = max_frames;
    s->la = stream_lookahead(pad, kP1TapReach);
    s->mel_ld = max_frames + 2 * pad;
    s->seed = h->seed;
    s->stream = h->stream_ctr;
    const size_t F = s->slots(), L = (size_t)max_frames * h->hop;
    CHECK(s->mel.alloc((size_t)h->feat * s->mel_ld * sizeof(float)));
    CHECK(s->act0.alloc((size_t)h->C * max_frames * sizeof(float)));
    CHECK(s->act1.alloc((size_t)h->C * max_frames * sizeof(float)));
    CHECK(s->Rb.alloc((size_t)h->R * max_frames * sizeof(float)));
    CHECK(s->q4.alloc(F * np * sizeof(float)));
    CHECK(s->a4.alloc(F * np * sizeof(float)));
    CHECK(s->fcond.alloc(F * cw * sizeof(float)));
    CHECK(s->st.alloc((size_t)kStreamState * sizeof(float)));
    CHECK(s->P1.alloc((size_t)np * sizeof(float)));
    CHECK(s->labels.alloc(L * sizeof(int16_t)));
    CHECK(s->samples.alloc(L * sizeof(float)));
    CHECK(h->stream_tab.alloc(4096));
    hipStream_t st = h->stream;
    // every slot that is not written yet holds NaN: a read ahead of the data shows as a wrong
    // label. The mel's leading pad columns and the front guard of p1q are the zeros they stand for.
    CHECK(fill_words(s->mel.p, kNaNWord, (size_t)h->feat * s->mel_ld, st));
    if (pad > 0)
        HIPC(hipMemset2DAsync(s->mel.p, (size_t)s->mel_ld * sizeof(float), 0, (size_t)pad * sizeof(float), h->feat, st));
    CHECK(fill_words(s->q4.p, kNaNWord, F * np, st));
    CHECK(fill_words(s->a4.p, kNaNWord, F * np, st));
    CHECK(fill_words(s->fcond.p, kNaNWord, F * cw, st));
    HIPC(hipMemsetAsync(s->q4.p, 0, (size_t)np * sizeof(float), st));
    HIPC(hipMemsetAsync(s->st.p, 0, (size_t)kStreamState * sizeof(float), st));
    CHECK(stream_zero_frame(s.get()));
    HIPC(hipStreamSynchronize(st));
    h->stream_ctr += 1u;
    h->sessions.push_back(s.get());
    *out = s.release();
    return WRNN_OK;
}

int wrnn_stream_push(wrnn_stream* s, const float* mel, int n_frames, int last) {
    if (!s) return fail(WRNN_ERR_INVALID, "null session");
    if (n_frames < 0 || (n_frames > 0 && !mel)) return fail(WRNN_ERR_INVALID, "bad mel");
    if (s->ended) return fail(WRNN_ERR_INVALID, "push after the last frames of the session");
    if (n_frames > s->max_frames - s->frames)
        return fail(WRNN_ERR_CAPACITY, "push of " + std::to_string(n_frames) + " frames past max_frames " +
                                           std::to_string(s->max_frames) + " (" + std::to_string(s->frames) + " pushed)");
    wrnn_handle* h = s->h;
    HIPC(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const int pad = h->cfg.pad, f0 = s->frames, f1 = f0 + n_frames;
    if (n_frames > 0)
        HIPC(hipMemcpy2DAsync(s->mel.f() + pad + f0, (size_t)s->mel_ld * sizeof(float), mel,
                              (size_t)n_frames * sizeof(float), (size_t)n_frames * sizeof(float), h->feat,
                              hipMemcpyHostToDevice, st));
    if (last && pad > 0)  // the zero padding behind the utterance, as the one-shot im2col applies it
        HIPC(hipMemset2DAsync(s->mel.f() + pad + f1, (size_t)s->mel_ld * sizeof(float), 0, (size_t)pad * sizeof(float),
                              h->feat, st));
    CHECK(stream_q_rows(s, f0, f1));
    const int a1 = last ? f1 : std::max(s->aux_done, f1 - pad);
    CHECK(stream_aux_rows(s, s->aux_done, a1));
    if (last)  // frames >= T read zeros: the two guard slots behind the last frame
        HIPC(hipMemsetAsync(s->q4.f() + (size_t)(kStreamFbase + 1 + f1) * 4 * h->H, 0, (size_t)2 * 4 * h->H * sizeof(float), st));
    HIPC(hipStreamSynchronize(st));  // (the caller's mel is free again)
    s->frames = f1;
    s->aux_done = a1;
    s->ended = last != 0;
    return WRNN_OK;
}

int wrnn_stream_advance(wrnn_stream* const* ss, int n, int16_t* const* labels, const size_t* capacity,
                        size_t* n_out) {
    if (n < 0 || (n > 0 && (!ss || !labels || !capacity || !n_out))) return fail(WRNN_ERR_INVALID, "null argument");
    if (n > kPG)
        return fail(WRNN_ERR_INVALID, "at most " + std::to_string(kPG) + " sessions per advance (one per XCD group)");
    for (int i = 0; i < n; ++i) {
        if (!ss[i]) return fail(WRNN_ERR_INVALID, "null session");
        if (ss[i]->h != ss[0]->h) return fail(WRNN_ERR_INVALID, "sessions of different handles in one advance");
        for (int j = 0; j < i; ++j)
            if (ss[j] == ss[i]) return fail(WRNN_ERR_INVALID, "a session listed twice in one advance");
    }
    if (n == 0) return WRNN_OK;
    int64_t run[kPG] = {0};
    int64_t max_run = 0;
    for (int i = 0; i < n; ++i) {
        run[i] = ss[i]->ready() - ss[i]->steps_done;
        if (run[i] > 0 && (!labels[i] || capacity[i] < (size_t)run[i]))
            return fail(WRNN_ERR_CAPACITY, "session " + std::to_string(i) + ": label capacity " +
                                               std::to_string(labels[i] ? capacity[i] : 0) + " < " +
                                               std::to_string(run[i]) + " ready steps");
        max_run = std::max(max_run, run[i]);
    }
    for (int i = 0; i < n; ++i) n_out[i] = 0;
    if (max_run <= 0) return WRNN_OK;  // nothing ready anywhere: no launch
    wrnn_handle* h = ss[0]->h;
    HIPC(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const auto& W = h->pw;
    const int np = 4 * h->H, ncls = h->n_classes, hop = h->hop;
    // the launch's tables: StreamGroup, row map, rows / steps per group, RowInfo -- by XCD group
    struct Tab {
        StreamGroup sg[kPG];
        int2 vmap[kPG];
        int gnr[kPG], giters[kPG];
        RowInfo rows[kPG];
    } tab;
    static_assert(sizeof(Tab) <= 4096, "stream_tab holds one launch's tables");
    std::memset(&tab, 0, sizeof(tab));
    for (int g = 0; g < kPG; ++g) tab.gnr[g] = 1;
    for (int i = 0; i < n; ++i) {
        wrnn_stream* s = ss[i];
        if (run[i] <= 0) continue;
        CHECK(s->gumbel.alloc((size_t)run[i] * ncls * sizeof(float)));
        StreamGroup& g = tab.sg[i];
        g.p1q = s->q4.f();
        g.p1a = s->a4.f();
        g.fcond = s->fcond.f();
        g.gumbel = s->gumbel.f();
        g.labels = (int16_t*)s->labels.p;
        g.samples = s->samples.f();
        g.st = s->st.f();
        g.P1 = s->P1.f();
        g.step0 = (int)s->steps_done;
        g.steps = (int)run[i];
        g.stream = s->stream;
        g.k0 = (uint32_t)(s->seed & 0xffffffffu);
        g.k1 = (uint32_t)(s->seed >> 32);
        tab.giters[i] = (int)run[i];
        RowInfo& ri = tab.rows[i];
        ri.pos0 = 0;
        ri.rel0 = g.step0;  // (as a rotated launch's table: the row's offset in its rel0)
        // before the last push no lookup of a running step may take the zero-frame branch
        ri.L = s->ended ? s->frames * hop : std::numeric_limits<int>::max() / 2;
        ri.fbase = kStreamFbase;
        ri.fold = 0;
        ri.stream = s->stream;
        // P1 of the first step, from the tables (k_p1_expand: position f0 * tpo + t = step0)
        HIPC(launch_p1_expand(s->P1.f(), 1, 0, 1, 1, 1, g.step0, ri.L, hop, s->ended ? s->frames : s->max_frames + 2,
                              np / 4, s->q4.f() + (size_t)kStreamFbase * np, s->a4.f() + (size_t)kStreamFbase * np,
                              W.p1taps, st));
        if (g.step0 == 0) {  // step 0 takes its state from zeros (k_persist_init)
            PersistArgs pi{};
            pi.B = 1;
            pi.P1 = s->P1.f();
            pi.b_hh1 = W.b_hh1;
            pi.b_hh2 = W.b_hh2;
            pi.st_x1 = s->st.f();
            pi.st_h1 = pi.st_x1 + kPH;
            pi.st_h2 = pi.st_h1 + kPH;
            pi.st_gh2 = pi.st_h2 + kPH;
            HIPC(launch_persist_init(pi, st));
        }
    }
    HIPC(hipMemcpyAsync(h->stream_tab.p, &tab, sizeof(tab), hipMemcpyHostToDevice, st));
    const char* tb = (const char*)h->stream_tab.p;
    const StreamGroup* sg_dev = (const StreamGroup*)(tb + offsetof(Tab, sg));
    HIPC(launch_stream_resume(sg_dev, n, h->v1, h->w0, st));
    HIPC(launch_gumbel_stream(sg_dev, n, (int)max_run, ncls, st));
    auto& P = h->pws;
    CHECK(P.ctl.alloc(PC_WORDS * sizeof(unsigned)));
    CHECK(P.xbuf.alloc(persist_xbuf_floats() * sizeof(float)));
    HIPC(hipMemsetAsync(P.ctl.p, 0, PC_WORDS * sizeof(unsigned), st));
    HIPC(hipMemsetAsync(P.xbuf.p, 0, persist_xbuf_floats() * sizeof(float), st));  // step tags
    PersistArgs a{};
    a.ctl = (unsigned*)P.ctl.p;
    a.xbuf = P.xbuf.f();
    a.t0 = 0;
    a.t1 = (int)max_run;
    a.S = 1 << 30;  // (no row ends inside a launch: the P1 look-ahead is bounded by RowInfo::L)
    a.B = 1;
    a.nr = 1;
    a.rb = 0;
    a.nreal = 1;
    a.mode = h->cfg.mode;
    a.n_classes = ncls;
    a.hop = hop;
    a.cpw = W.cpw;
    a.rows = (const RowInfo*)(tb + offsetof(Tab, rows));
    a.wreg = (const float4*)W.wreg;
    a.wlds = (const float4*)W.wlds;
    a.b_hh1 = W.b_hh1;
    a.b_hh2 = W.b_hh2;
    a.b_fc3 = W.b_fc3;
    a.v = h->v1;
    a.w0 = h->w0;
    a.cond_width = h->cond_width;
    a.oG2 = W.oG2;
    a.oF1 = W.oF1;
    a.oF2 = W.oF2;
    a.p1taps = W.p1taps + (size_t)hop * 8;  // the [hop][4] table
    a.p1split = W.p1split;
    a.ld = 0;
    a.phase_t = -1;
    a.vmap = (const int2*)(tb + offsetof(Tab, vmap));
    a.gnr = (const int*)(tb + offsetof(Tab, gnr));
    a.giters = (const int*)(tb + offsetof(Tab, giters));
    a.sgroup = sg_dev;
    const hipError_t le = launch_persist_stream(a, st);
    if (le != hipSuccess) {
        (void)hipStreamSynchronize(st);
        return fail(WRNN_ERR_HIP, le == hipErrorCooperativeLaunchTooLarge
                                      ? std::string("streaming launch: workgroups cannot become co-resident")
                                      : std::string("streaming launch: ") + hipGetErrorString(le));
    }
    for (int i = 0; i < n; ++i)
        if (run[i] > 0)
            HIPC(hipMemcpyAsync(labels[i], ss[i]->labels.p, (size_t)run[i] * sizeof(int16_t), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    unsigned err = 0;
    HIPC(hipMemcpy(&err, (unsigned*)P.ctl.p + PC_ERR, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (err) {
        static const char* what[] = {"", "workgroups did not become co-resident", "exchange timeout",
                                     "workgroups not spread 32 per XCD", "aborted"};
        return fail(WRNN_ERR_HIP, std::string("streaming launch: ") + (err < 5 ? what[err] : "unknown error"));
    }
    for (int i = 0; i < n; ++i)
        if (run[i] > 0) {
            ss[i]->steps_done += run[i];
            n_out[i] = (size_t)run[i];
        }
    return WRNN_OK;
}

int wrnn_stream_status(wrnn_stream* s, int* frames_pushed, int* ended, int64_t* steps_done, int64_t* steps_ready,
                       int* lookahead_frames) {
    if (!s) return fail(WRNN_ERR_INVALID, "null session");
    if (frames_pushed) *frames_pushed = s->frames;
    if (ended) *ended = s->ended ? 1 : 0;
    if (steps_done) *steps_done = s->steps_done;
    if (steps_ready) *steps_ready = s->ready();
    if (lookahead_frames) *lookahead_frames = s->la;
    return WRNN_OK;
}

void wrnn_stream_close(wrnn_stream* s) {
    if (!s) return;
    wrnn_handle* h = s->h;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    h->sessions.erase(std::remove(h->sessions.begin(), h->sessions.end(), s), h->sessions.end());
    delete s;
}

static int copy_row(const DevBuf& q, const DevBuf& a, const DevBuf& fc, wrnn_handle* h, size_t slot, size_t slots,
                    int table, float* out, size_t capacity, int* width) {
    if (table < 0 || table > 2) return fail(WRNN_ERR_INVALID, "table must be 0 (p1q), 1 (p1a) or 2 (fcond)");
    const size_t w = table == 2 ? (size_t)h->cond_width : (size_t)4 * h->H;
    const DevBuf& b = table == 0 ? q : table == 1 ? a : fc;
    if (width) *width = (int)w;
    if (!b.p || slot >= slots || (slot + 1) * w * sizeof(float) > b.bytes) return fail(WRNN_ERR_INVALID, "frame out of range");
    if (!out || capacity < w) return fail(WRNN_ERR_CAPACITY, "row capacity");
    HIPC(hipMemcpy(out, b.f() + slot * w, w * sizeof(float), hipMemcpyDeviceToHost));
    return WRNN_OK;
}

int wrnn_debug_stream_row(wrnn_stream* s, int frame, int table, float* out, size_t capacity, int* width) {
    if (!s) return fail(WRNN_ERR_INVALID, "null session");
    if (frame < -1 || frame >= s->max_frames) return fail(WRNN_ERR_INVALID, "frame out of range");
    HIPC(hipSetDevice(s->h->device));
    HIPC(hipStreamSynchronize(s->h->stream));
    return copy_row(s->q4, s->a4, s->fcond, s->h, (size_t)(kStreamFbase + 1 + frame), s->slots(), table, out, capacity, width);
}

int wrnn_debug_frame_row(wrnn_handle* h, int frame, int table, float* out, size_t capacity, int* width) {
    if (!h) return fail(WRNN_ERR_INVALID, "null handle");
    if (h->last_engine != WRNN_ENGINE_PERSIST || !h->p1_ring || h->rows_host.empty())
        return fail(WRNN_ERR_INVALID, "the last call did not run the persistent engine with per-frame tables");
    if (frame < -1 || frame >= h->last_T0) return fail(WRNN_ERR_INVALID, "frame out of range");
    HIPC(hipSetDevice(h->device));
    HIPC(hipStreamSynchronize(h->stream));
    return copy_row(h->ws.q4, h->ws.a4, h->ws.fcond, h, (size_t)(h->rows_host[0].fbase + 1 + frame), (size_t)h->ws.Fcap,
                    table, out, capacity, width);
}

}  // extern "C"
