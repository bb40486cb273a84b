// Persistent geneing recurrence for WIDE row batches (launch kind "persist-wide" of the geneing
// topology): up to 16 fold rows per XCD group, 128 rows per launch, every product on the fp32
// matrix cores (v_mfma_f32_16x16x4_f32). Three heads, each its own instantiation (template
// parameter MODE): geneing 'BITS' (WRNN_MODE_RAW, 512 or 1024 classes), MOL (30 logits, mixture of
// logistics) and Beta (geneing 'RAW', WRNN_MODE_BETA, 2 logits). Calls of at most 32 rows stay on
// k_persist_gen (the planner offers this kernel above that, or under WRNN_PERSIST_WIDE=1). The
// 32-row ring instances (k_persist_wide_gen32, below the 16-row kernel: two column tiles per group,
// 256 rows per launch) are opt-in (wrnn_set_gen_wide_rows), and so are the time-sliced ring
// instances (k_persist_wide_gen_rot, between the two: launches of 16 rows per group over rotating
// row sets; wrnn_set_gen_wide_slices).
//
// Reference step body: vocoder/models/geneing_version.py:193-205 (rnn_dims 256, fc_dims 128):
//   x1 = I(x0) + h1'     h1' = rnn1(I(x0), h1)
//   y1 = relu(fc1([x1, a2]))        logits = fc3(y1) -> categorical draw
// restructured as kernels_persist_gen.hip (conditioning per frame, P1 + v x for GRU1's input,
// torch-form gate math with contraction off).
//
// Layout: the 32 slots of an XCD group are alike (no halves: the step is one chain, so a split
// in two halves would leave one half idle and give each busy slot twice the tiles). Slot w owns
// GRU units [8 w, 8 w + 8), fc1 outputs [4 w, 4 w + 4) and fc3 classes [cpw w, cpw (w + 1)),
// cpw = n / 32 (16 or 32). Its five MFMA A tiles (16 rows each):
//   T0  W_hh1 gate r of the 8 units (m < 8) | gate z (m >= 8)          K = 256
//   T1  W_hh1 gate n of the 8 units (m < 8) | zero                     K = 256
//   T2  fc1[:, :256] rows 4 w + m (m < 4) | zero                       K = 256
//   T3, T4  fc3 rows cpw w + 16 j + m (j < cpw / 16)                   K = 128
// (T1 and T2 are half and three quarters empty: 32 MFMAs per wave and step in all, against 40
// for a two-half split with full tiles.) K is split over the 8 waves (K = 256: wave v takes
// inputs [32 v, 32 v + 32), 8 k-steps of 4; K = 128: [16 v, 16 v + 16), 4 k-steps), the 8
// partial tiles are summed in LDS in a fixed order (v = 0 .. 7) by the epilogue lanes: cell
// (row cn, column cul) = thread 16 cn + cul on waves 0-3. Weights stay in 32 VGPRs per lane for
// the whole launch.
//
// Three exchanges lie on a step's dependency chain, W_hh1 h1 runs in a wait:
//   poll x1 -> fc1 -> y1 (hop 1) | poll h1 -> W_hh1 h1 (while the other slots' y1 arrive)
//   poll y1 -> fc3 -> per-slot candidate keys (hop 2)
//   poll the 32 candidates of every row -> sample, GRU1 of step t + 1 for the slot's units ->
//   x1, h1 (hop 3)
// Vectors travel as 16-byte packets in MFMA B-operand order, untagged, with a sentinel-reset
// slot pair per vector (the protocol of kernels_persist_wide_rr.hip; DESIGN.md §3.0d, the
// buffer-ordering table of this kernel is in §3.0c). Candidates are the two-word keys of
// cand_key.h, tagged with the step. Stream instances (RING false) read the Gumbel noise [S][B][n]
// and P1 [S][B][256][4] from the call's streams as k_persist_gen reads them: a 64-bit base per step
// (uniform) plus a 32-bit offset inside the step. Ring instances (RING true; calls whose launches
// are all wide) form both in-kernel: waves 4-7, which own no epilogue cell, write the slot's P1
// (ring_p1_make, from the per-frame tables) and its Gumbel words (ring_noise_make, BITS only) into one-slot
// LDS arrays that waves 0-3 read -- every value is produced and consumed by the same workgroup, so
// the two workgroup barriers of the step order them and nothing new crosses workgroups.
//
// MOL / Beta (MODE 1 / 2): fc3 has 30 / 2 outputs, so it is one 16-row tile per slot (cpw = 16):
// slots 0 and 1 hold logit rows 16 w + m (Beta: slot 0 rows 0 and 1), every other slot runs the
// tile on a zero image, so all 32 slots still poll x1, h1 and y1 and the sentinel protocol of the
// vectors is exactly BITS's. No Gumbel stream is read and no candidate is formed: the fc3
// epilogue of the owning slots publishes each (row, logit) as a tagged pair (float bits, the whole
// step tag seq = t + 1) into the candidate area, which has exactly the shape [16 rows][32] pairs
// and is zeroed before every launch (g_logit; wide_gen_mol_layout_check). In hop 3 lane cul of a
// row polls logits cul and 16 + cul of its row, bounded like every other spin, and every slot
// forms the sample redundantly (each needs x for its own GRU units); slot 0 writes `samples`,
// there are no labels. The area is single-buffered like the candidates: a slot publishes the
// logits of step t + 1 only after y1 of t + 1 of every slot, which follows x1 of t + 1 of every
// slot, which every slot publishes after its hop 3 of step t.
//   MOL:  k_persist_gen's operations in its order (persist_wide_common.h mol_sample_row16: first
//         max over the 10 mixture logits minus their draws, mean, log-scale clamp,
//         mean + exp(ls) lu, clamp to [-1, 1]); the 11 draws of
//         a row come from the k_mol_noise stream [S][B][kMolNoise], lane cul holds draw cul,
//         loaded one step ahead.
//   Beta: lanes 0 and 1 of a row draw X ~ Gamma(exp l0), Y ~ Gamma(exp l1) concurrently (philox.h
//         gamma_mt, keyed by the row's step, fold and stream), lane 0 forms 2 X / (X + Y) - 1.
//
// One step body for both kernels: k_persist_wide_gen (16 rows) and k_persist_wide_gen32 (32 rows)
// call the same step pieces (gen_* below, on a GenCell and the LDS layout GenLds<tiles>); a kernel
// keeps only what differs, its MFMA loops over one or two column tiles and its ring work. The
// helpers shared with the other wide kernels (sentinel, polls, samplers, timeout report) are in
// persist_wide_common.h.
#include "wrnn_kernels.h"
#include "persist_wide_common.h"
#include "philox.h"

#include <type_traits>
#include <vector>

namespace wrnn {
namespace {

constexpr int GH = kRH;        // rnn_dims 256
constexpr int GF = kGF;        // fc_dims 128
constexpr int GU = GH / kPM;   // GRU units per slot (8)
constexpr int GO = GF / kPM;   // fc1 outputs per slot (4)
constexpr int kRowsW = 16;     // rows per group and column tile (MFMA N)

// ---- exchange area per group (floats) ---------------------------------------------------
// x1, h1 (256 units): per step parity slot [e 8][p 2][lane 64] packets of 4 floats; packet p of
// consumer lane l = 16 c + n of wave e holds row n, units 32 e + 8 c + 4 p + q (q < 4)
// y1 (128 units): [e 8][lane 64] packets; lane l = 16 c + n of wave e: row n, units 16 e + 4 c + q
constexpr int GS_X = 8 * 2 * 64 * 4;
constexpr int GS_Y = 8 * 64 * 4;
constexpr int GX_X1 = 0, GX_H1 = GX_X1 + 2 * GS_X, GX_Y1 = GX_H1 + 2 * GS_X;
constexpr int GX_D = GX_Y1 + 2 * GS_Y;  // candidates [row 16][slot 32] (key hi, key lo | tag)
constexpr int GX_GROUP = GX_D + kRowsW * kPM * 2 + 64;
static_assert(GX_GROUP % 4 == 0 && GX_D % 4 == 0, "reset works in 16-byte units");
// 32-row instances: tile 1 (rows 16-31) has its own copy of the whole area behind tile 0's
constexpr int kRows32 = 2 * kRowsW;
constexpr unsigned kTile1B = (unsigned)GX_GROUP * 4u;  // byte offset of tile 1's copy in a group's area
constexpr int GX_GROUP32 = 2 * GX_GROUP;
static_assert(kTile1B % 16 == 0, "tile 1's copy: 16-byte aligned");

__host__ __device__ constexpr unsigned g_cons_x(int v, int l) { return (unsigned)((v * 2 * 64 + l) * 16); }
__host__ __device__ constexpr unsigned g_cons_y(int v, int l) { return (unsigned)((v * 64 + l) * 16); }
// packet of the unit quad u .. u + 3 (u % 4 == 0) of row cn
__host__ __device__ constexpr unsigned g_prod_x(int u, int cn) {
    return (unsigned)((((u >> 5) * 2 + ((u >> 2) & 1)) * 64 + 16 * ((u >> 3) & 3) + cn) * 16);
}
__host__ __device__ constexpr unsigned g_prod_y(int u, int cn) {
    return (unsigned)(((u >> 4) * 64 + 16 * ((u >> 2) & 3) + cn) * 16);
}
// byte offset of parity slot seq & 1 of the vector at float offset `buf` (slots of `sz` floats)
__host__ __device__ constexpr unsigned g_slot(int buf, int sz, unsigned seq) {
    return (unsigned)buf * 4u + (seq & 1u) * (unsigned)sz * 4u;
}
__host__ __device__ constexpr unsigned g_cand(int n, int s) { return (unsigned)((n * kPM + s) * 2) * 4u; }
// MOL / BETA launches publish no candidate: the area holds the rows' logits instead, logit k
// (< 30 or 2) of row n as a tagged pair (float bits, the whole step tag seq = t + 1) at the
// place of the candidate of "slot" k; byte offset inside the area (wide_gen_mol_layout_check)
constexpr int kGenLogitsMax = 32;
__host__ __device__ constexpr unsigned g_logit(int n, int k) { return (unsigned)((n * kGenLogitsMax + k) * 2) * 4u; }
static_assert(kGenLogitsMax == kPM && g_logit(kRowsW - 1, kGenLogitsMax - 1) + 8 == (unsigned)(kRowsW * kPM * 2) * 4u,
              "the logit pairs fill the candidate area");

// ---- LDS (floats), for NT column tiles of 16 rows (1: the 16-row kernel, 2: the 32-row one) ----
constexpr int WT = 8 * 256;  // the 8 waves' partials of one 16 x 16 tile
constexpr int kGrW = 32;     // Gumbel words per row in the ring's noise array
template <int NT>
struct GenLds {
    static constexpr int kRows = NT * kRowsW;
    static constexpr int RI = 0;                             // RowInfo of the group's rows (6 words each)
    static constexpr int FAIL = NT == 1 ? 112 : 6 * kRows;   // behind the RowInfo array
    static constexpr int REG = FAIL + 4;                     // group, slot, registration result (ints)
    static constexpr int CB = REG + 12;  // b_hh1 of the slot's units [3][8], then b_f3 of its classes @32
    // time-sliced launches: (physical row, step offset) of the group's rows, as int2
    static constexpr int VM = CB + 64;
    // partial tiles [tile][8 v][nt][16 n][16 m], one buffer per product (fc1: nt 1, W_hh1 and fc3: 2)
    static constexpr int P = 256 * NT;
    static constexpr int F1 = P, HH = F1 + NT * WT, F3 = HH + 2 * NT * WT, TOTAL = F3 + 2 * NT * WT;
    // ring instances: P1 of the next step as float4 [n][8 units], the step's Gumbel words
    // [n][32 (cpw 16: the first 16)] -- one slot each, behind the partial tiles
    static constexpr int P1R = TOTAL, GR = P1R + kRows * GU * 4, TOTAL_RING = GR + kRows * kGrW;
    static_assert(sizeof(RowInfo) == 24 && kRows * 6 <= FAIL, "RowInfo array overflows");
    static_assert(CB + 32 + 32 <= P && REG % 4 == 0, "slot constants overflow");
    static_assert(VM % 2 == 0 && VM + 2 * kRowsW <= P, "virtual-row map overflows");
    static_assert(P % 4 == 0 && P1R % 4 == 0 && WT % 4 == 0, "partial tiles and P1 array: float4-aligned");
    static_assert(TOTAL_RING * sizeof(float) <= (NT == 1 ? 64 : 160) * 1024, "LDS arrays exceed the kernel's carve");
};
// the 32-row layout is the 16-row one with every per-tile and per-row array doubled, in the same order
static_assert(GenLds<2>::P == 2 * GenLds<1>::P && GenLds<2>::HH - GenLds<2>::F1 == 2 * (GenLds<1>::HH - GenLds<1>::F1) &&
                  GenLds<2>::F3 - GenLds<2>::HH == 2 * (GenLds<1>::F3 - GenLds<1>::HH) &&
                  GenLds<2>::TOTAL - GenLds<2>::P == 2 * (GenLds<1>::TOTAL - GenLds<1>::P) &&
                  GenLds<2>::TOTAL_RING - GenLds<2>::P == 2 * (GenLds<1>::TOTAL_RING - GenLds<1>::P),
              "GenLds<2> doubles GenLds<1>'s arrays");

constexpr int kWgq = 8;  // float4 weight registers per lane: T0-T2 two each, T3, T4 one each

// ---- a thread's place in the step -----------------------------------------------------------
// Workgroup (group g, slot w), wave v (K-eighth v of every product), lane l, MFMA column bn, and
// the epilogue cell: row cn of the group = column cnl of tile tt, tile row cul. 16-row kernel: the
// cells lie on waves 0-3, tt = 0; 32-row kernel: tile 1's cells on waves 4-7. xt: byte offset of
// the cell's tile copy in the group's exchange area (0 for tile 0).
template <int NT>
struct GenCell {
    using L = GenLds<NT>;
    float* lds;
    rsrc_t xr;
    int g, w, v, l, bn, R, g0;
    int tt, cn, cnl, cul, cu, crow;
    unsigned xt;
    bool cell, gcell, fcell;
    int ntc;              // fc3 tiles of the slot (1 or 2; MOL / BETA: 1)
    unsigned o_px, o_py;  // publishing lanes: x1 / h1 the first lane of each unit quad, y1 the row's lane 0

    __device__ __forceinline__ unsigned wh(unsigned site) const { return site << 28 | (unsigned)w << 22; }
    __device__ __forceinline__ const RowInfo& row(int n) const {
        return reinterpret_cast<const RowInfo*>(lds + L::RI)[n];
    }
    // publish the lane's value of step seq as one packet of its quad: slot seq & 1, the
    // sentinel into slot (seq + 1) & 1. Every lane of the wave issues both stores (a lane that
    // does not publish uses kNoOff, which the buffer range check drops): no branch around them,
    // so the compiler's waits after them stay counted
    __device__ __forceinline__ void pub(int buf, int sz, unsigned off, float val, unsigned seq) const {
        const float u1 = pdpp<0x39>(val), u2 = pdpp<0x4E>(val), u3 = pdpp<0x93>(val);
        unsigned vo = off;
        asm volatile("" : "+v"(vo));
        __builtin_amdgcn_raw_buffer_store_b128(
            (u4v){__float_as_uint(val), __float_as_uint(u1), __float_as_uint(u2), __float_as_uint(u3)}, xr, vo,
            g_slot(buf, sz, seq) + xt, 0);
        __builtin_amdgcn_raw_buffer_store_b128((u4v){kSent, kSent, kSent, kSent}, xr, vo,
                                               g_slot(buf, sz, seq + 1u) + xt, 0);
    }
    // partial tile j (of nt) of a product, column tile `tile`, into P ([tile][v][nt][n][m], swizzled)
    __device__ __forceinline__ void put(int P, int nt, int tile, int j, const v4f& acc) const {
        *reinterpret_cast<v4f*>(lds + P + tile * nt * WT + ((v * nt + j) * 16 + bn) * 16 + wsw(bn, 4 * (l >> 4))) = acc;
    }
    // the cell's sum of the 8 waves' partials of tile j, tile row m (fixed order v = 0 .. 7)
    __device__ __forceinline__ float psum(int P, int nt, int j, int m) const {
        float p[8];
#pragma unroll
        for (int vv = 0; vv < 8; ++vv) p[vv] = lds[P + tt * nt * WT + ((vv * nt + j) * 16 + cnl) * 16 + wsw(cnl, m)];
        float acc = 0.f;
#pragma unroll
        for (int vv = 0; vv < 8; ++vv) acc += p[vv];
        return acc;
    }
};

// registration of the workgroup; false: the launch is not to run (p_register)
template <class L>
__device__ __forceinline__ bool gen_register(unsigned* ctl, float* lds, int& g, int& w) {
    int* sreg = reinterpret_cast<int*>(lds + L::REG);
    if (threadIdx.x == 0) {
        int gg, ss;
        sreg[2] = p_register(ctl, gg, ss);
        sreg[0] = gg;
        sreg[1] = ss;
    }
    __syncthreads();
    if (!sreg[2]) return false;
    g = __builtin_amdgcn_readfirstlane(sreg[0]);
    w = __builtin_amdgcn_readfirstlane(sreg[1]);
    return true;
}

template <int MODE, int NT>
__device__ __forceinline__ GenCell<NT> gen_cell(const PersistGenArgs& a, float* lds, int g, int w) {
    GenCell<NT> c;
    const int tid = threadIdx.x;
    c.lds = lds;
    c.g = g;
    c.w = w;
    c.v = __builtin_amdgcn_readfirstlane(tid >> 6);
    c.l = tid & 63;
    c.bn = c.l & 15;
    c.R = a.nr;
    c.g0 = a.rb + g;
    c.tt = NT == 1 ? 0 : c.v >> 2;
    c.cn = tid >> 4;
    c.cnl = NT == 1 ? c.cn : c.cn & 15;
    c.cul = tid & 15;
    c.cell = NT == 1 ? tid < 16 * c.R : c.cn < c.R;
    c.gcell = c.cell && c.cul < GU;  // GRU cell: unit 8 w + cul
    c.fcell = c.cell && c.cul < GO;  // fc1 cell: output 4 w + cul
    c.cu = GU * w + (c.cul & 7);
    c.crow = c.g0 + kPG * (c.cell ? c.cn : 0);
    c.ntc = MODE == 0 ? a.cpw / 16 : 1;
    c.xr = mk_rsrc(a.xbuf + (size_t)g * (NT * GX_GROUP));
    c.xt = (unsigned)c.tt * kTile1B;  // (uniform)
    c.o_px = c.gcell && (c.cul & 3) == 0 ? g_prod_x(GU * w + c.cul, c.cnl) : kNoOff;
    c.o_py = c.cell && c.cul == 0 ? g_prod_y(GO * w, c.cnl) : kNoOff;
    return c;
}

// ---- weights: K = 256 tile T (< 3), k-step ks at wq[2 T + ks / 4] component ks % 4;
//      fc3 tile j, k-step ks at wq[6 + j] component ks -------------------------------------
template <int NT>
__device__ __forceinline__ void gen_load_weights(const PersistGenArgs& a, const GenCell<NT>& c, float4 (&wq)[kWgq]) {
    const float4* src = a.wwide + ((size_t)(c.w * 8 + c.v) * kWgq) * 64 + c.l;
#pragma unroll
    for (int q = 0; q < kWgq; ++q) wq[q] = src[(size_t)q * 64];
}
// the group's RowInfo and the slot's biases into LDS, the failure flag cleared
template <int NT>
__device__ __forceinline__ void gen_setup_lds(const PersistGenArgs& a, const GenCell<NT>& c) {
    using L = GenLds<NT>;
    const int tid = threadIdx.x;
    float* lds = c.lds;
    if (tid < c.R) reinterpret_cast<RowInfo*>(lds + L::RI)[tid] = a.rows[c.g0 + kPG * tid];
    if (tid == 0) lds[L::FAIL] = 0.f;
    if (tid < 24) lds[L::CB + tid] = a.b_hh1[(tid >> 3) * GH + GU * c.w + (tid & 7)];
    if (tid >= 32 && tid < 32 + a.cpw) {
        const int cl = a.cpw * c.w + tid - 32;
        lds[L::CB + tid] = cl < a.n_classes ? a.b_f3[cl] : 0.f;
    }
}

// what a cell carries over the launch: its GRU unit's state and input weights, and (MOL / BETA)
// its places in the draw stream and the logit-pair area
struct GenState {
    float h1r, x1c;
    float vr, vz, vn, w0c;
    // MOL: lane cul < kMolNoise of a row holds draw cul of its row from the k_mol_noise stream
    // ([S][B][kMolNoise]); pg is the draw of step t, pgn the one of step t + 1 (clamped at the
    // last step, where it goes unused)
    float pg, pgn;
    unsigned o_mol;
    // MOL / BETA: the lane's pair in the logit area as producer (slots 0 and 1: logit 16 w + cul)
    // and as consumer (logits cul and 16 + cul of row cn); kNoOff where there is none
    bool l_ra, l_rb;
    unsigned o_lp;
};
template <int NT>
__device__ __forceinline__ GenState gen_state(const PersistGenArgs& a, const GenCell<NT>& c) {
    GenState s;
    s.h1r = 0.f;
    s.x1c = 0.f;
    if (c.gcell) {  // x1, h1 of step 0 (k_persist_gen_init)
        const float* st = a.st + (size_t)c.crow * 2 * GH;
        s.x1c = st[c.cu];
        s.h1r = st[GH + c.cu];
    }
    s.vr = c.gcell ? a.v[c.cu] : 0.f;
    s.vz = c.gcell ? a.v[GH + c.cu] : 0.f;
    s.vn = c.gcell ? a.v[2 * GH + c.cu] : 0.f;
    s.w0c = c.gcell ? a.w0[c.cu] : 0.f;
    s.pg = 0.f;
    s.pgn = 0.f;
    s.o_mol = (unsigned)(c.crow * kMolNoise + c.cul) * 4u;
    s.l_ra = c.cell && c.cul < a.n_classes;
    s.l_rb = c.cell && 16 + c.cul < a.n_classes;
    s.o_lp = c.cell && c.w < 2 && 16 * c.w + c.cul < a.n_classes ? g_logit(c.cnl, 16 * c.w + c.cul) : kNoOff;
    return s;
}
// MOL: the row's draws of step te into pgn. ROT (time-sliced launch): te counts from the row's
// offset `off`, so the step's base differs between the rows of a wave and the whole address is a
// 32-bit offset into the stream (the planner and the launcher hold such a call's stream to 2 GiB)
template <int NT, bool ROT = false>
__device__ __forceinline__ void gen_mol_draw(const PersistGenArgs& a, const GenCell<NT>& c, GenState& s, int te,
                                             int off = 0) {
    if constexpr (ROT) {
        const int tc = te < a.S - off ? te : a.S - off - 1;
        if (c.cell && c.cul < kMolNoise)
            s.pgn = bld(mk_rsrc(a.gumbel), (unsigned)((tc + off) * a.B * kMolNoise) * 4u + s.o_mol, 0);
    } else {
        const int tc = te < a.S ? te : a.S - 1;
        if (c.cell && c.cul < kMolNoise) s.pgn = bld(mk_rsrc(a.gumbel + (size_t)tc * a.B * kMolNoise), s.o_mol, 0);
    }
}
// initial x1, h1 (canonicalised: a signalling NaN in a carried state must not read as the
// sentinel), as step t0's vectors
template <int NT>
__device__ __forceinline__ void gen_pub_initial(const PersistGenArgs& a, const GenCell<NT>& c, const GenState& s) {
    c.pub(GX_X1, GS_X, c.o_px, __builtin_canonicalizef(s.x1c), (unsigned)a.t0 + 1u);
    c.pub(GX_H1, GS_X, c.o_px, __builtin_canonicalizef(s.h1r), (unsigned)a.t0 + 1u);
}
// fc1 conditioning of frame(t) for the cell's output
template <int NT>
__device__ __forceinline__ float gen_fc1_cond(const PersistGenArgs& a, const GenCell<NT>& c, rsrc_t fcr, int t) {
    float pc = 0.f;
    if (c.fcell)
        pc = bld(fcr, (unsigned)(p_frame(c.row(c.cn), t, a.hop) * a.cond_width + a.oF1 + GO * c.w + c.cul) * 4u, 0);
    return pc;
}
// y1 = relu(fc1 partials + conditioning) of the cell's output, published (hop 1's end)
template <int NT>
__device__ __forceinline__ void gen_pub_y1(const GenCell<NT>& c, float pc, unsigned seq) {
    float y = 0.f;
    if (c.fcell) {
        y = p_add(c.psum(GenLds<NT>::F1, 1, 0, c.cul), pc);
        y = y > 0.f ? y : 0.f;
    }
    c.pub(GX_Y1, GS_Y, c.o_py, y, seq);
}
// ring instances: the cell's noise of step t and P1(t + 1) from the one-slot LDS arrays: written
// before the step's first barrier (the step before, or the prologue), overwritten only after its
// second
template <int MODE, int NT>
__device__ __forceinline__ void gen_ring_read(const GenCell<NT>& c, float (&pn)[2], float4& pp) {
    using L = GenLds<NT>;
    if constexpr (MODE == 0) {
        if (c.cell) {
            pn[0] = c.lds[L::GR + c.cn * kGrW + c.cul];
            if (c.ntc == 2) pn[1] = c.lds[L::GR + c.cn * kGrW + 16 + c.cul];
        }
    }
    if (c.gcell) pp = reinterpret_cast<const float4*>(c.lds + L::P1R)[c.cn * GU + c.cul];
}
// fc3 epilogue (hop 2's end), from the partials in F3
template <int MODE, bool DBG, int NT>
__device__ __forceinline__ void gen_pub_fc3(const PersistGenArgs& a, const GenCell<NT>& c, const GenState& s,
                                            const float (&pn)[2], int t, unsigned seq, int off = 0) {
    using L = GenLds<NT>;
    const float* cb = c.lds + L::CB;
    if constexpr (MODE == 0) {
        // candidate: the max key (cand_key.h cand_key, l_k + G_k formed exactly) over the
        // slot's classes of row cn: lane cul takes classes cpw w + 16 j + cul, j < ntc
        uint32_t kh = 0, kl = 0;
        if (c.cell) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (j >= c.ntc) break;
                const int cl = a.cpw * c.w + 16 * j + c.cul;
                const float lg = p_add(c.psum(L::F3, 2, j, c.cul), cb[32 + 16 * j + c.cul]);
                p_dbg_logit<DBG>(a.dbg, t + off, c.crow, cl, a.B, a.n_classes, lg);
                const CandKey k = cand_key(lg, __float_as_uint(pn[j]), cl);
                kmax_take(kh, kl, k.hi, k.lo);
            }
        }
        row16_kmax(kh, kl);
        unsigned vo = c.cell && c.cul == 0 ? g_cand(c.cnl, c.w) : kNoOff;
        asm volatile("" : "+v"(vo));
        __builtin_amdgcn_raw_buffer_store_b64((u2v){kh, kl | key_tag(seq)}, c.xr, vo, GX_D * 4 + c.xt, 0);
    } else {
        // MOL / BETA: logit 16 w + cul of row cn (slots 0 and 1) as a tagged pair (float
        // bits, seq), polled directly in hop 3; every lane issues the store (kNoOff: dropped)
        float lg = 0.f;
        if (s.o_lp != kNoOff) {
            lg = p_add(c.psum(L::F3, 2, 0, c.cul), cb[32 + c.cul]);
            p_dbg_logit<DBG>(a.dbg, t + off, c.crow, 16 * c.w + c.cul, a.B, a.n_classes, lg);
        }
        unsigned vo = s.o_lp;
        asm volatile("" : "+v"(vo));
        __builtin_amdgcn_raw_buffer_store_b64((u2v){__float_as_uint(lg), seq}, c.xr, vo, GX_D * 4 + c.xt, 0);
    }
}
// gh1 = W_hh1 h1 + b_hh1 of the cell's unit, from the partials in HH
template <int NT>
__device__ __forceinline__ void gen_gh1(const GenCell<NT>& c, float& g1r, float& g1z, float& g1n) {
    using L = GenLds<NT>;
    const float* cb = c.lds + L::CB;
    g1r = g1z = g1n = 0.f;
    if (c.gcell) {
        g1r = p_add(c.psum(L::HH, 2, 0, c.cul), cb[c.cul]);
        g1z = p_add(c.psum(L::HH, 2, 0, 8 + c.cul), cb[8 + c.cul]);
        g1n = p_add(c.psum(L::HH, 2, 1, c.cul), cb[16 + c.cul]);
    }
}
// ---- hop 3: the sample of step t; slot 0 stores it (BITS: with its label). Every slot forms it
// (each needs x for its own GRU units). BITS: lane cul polls the candidates of slots 2 cul,
// 2 cul + 1 of row cn; MOL / BETA: logits cul and 16 + cul of its row. ROT (time-sliced launch):
// t is the launch's step and the row's own step is t + off -- the column of its outputs, which go
// to its physical row (the virtual-row map in LDS), and the step of its Beta draws -------------
template <int MODE, int NT, bool ROT = false>
__device__ __forceinline__ float gen_sample(const PersistGenArgs& a, const GenCell<NT>& c, GenState& s, int t,
                                            unsigned seq, bool& fail, int off = 0) {
    float x;
    auto out_row = [&](int nn) {  // the call's row of the group's slot nn
        if constexpr (ROT) return reinterpret_cast<const int2*>(c.lds + GenLds<NT>::VM)[nn].x;
        else return c.g0 + kPG * nn;
    };
    if constexpr (MODE == 0) {
        u4v q;
        fail |= !poll_cand_couple(c.xr, c.cell, g_cand(c.cnl, 2 * c.cul), GX_D * 4 + c.xt, key_tag(seq), a.ctl,
                                  c.wh(4), (unsigned)t, true, q);
        uint32_t bh = c.cell ? q.x : 0u, bl = c.cell ? q.y : 0u;
        kmax_take(bh, bl, c.cell ? q.z : 0u, c.cell ? q.w : 0u);
        row16_kmax(bh, bl);  // the 32 slots' candidates: argmax over all classes of row cn
        const int bi = key_cls(bl);
        x = bits_sample_of(bi, a.n_classes);
        if (c.w == 0 && c.cell && c.cul == 0) {
            int nn = c.cn;
            asm volatile("" : "+v"(nn));
            const unsigned ro = (unsigned)(out_row(nn) * a.ld);
            __builtin_amdgcn_raw_buffer_store_b16((unsigned short)bi, mk_rsrc(a.labels), ro * 2u,
                                                  (unsigned)(t + off) * 2u, 0);
            bst(x, mk_rsrc(a.samples), ro * 4u, (unsigned)(t + off) * 4u);
        }
    } else {
        u2v qa, qb;
        fail |= !poll_logit_pairs(c.xr, s.l_ra ? g_logit(c.cnl, c.cul) : kNoOff,
                                  s.l_rb ? g_logit(c.cnl, 16 + c.cul) : kNoOff, GX_D * 4 + c.xt, s.l_ra, s.l_rb, seq,
                                  a.ctl, c.wh(5), (unsigned)t, true, qa, qb);
        const float la = __uint_as_float(qa.x);
        [[maybe_unused]] const float lb = __uint_as_float(qb.x);
        if constexpr (MODE == 2) {
            // BETA (geneing 'RAW'): vocoder/distribution.py:7-20, Beta(exp l0, exp l1) on
            // [-1, 1] with the Philox gamma draws: lane 0 of the row draws X ~ Gamma(exp l0),
            // lane 1 Y ~ Gamma(exp l1) concurrently (philox.h gamma_mt, g = lane); lane 0
            // forms 2 X / (X + Y) - 1 exactly as beta_sample and k_persist_gen do
            const int base = c.l & 48;  // lane 0 of this lane's row
            double gv = 0.0;
            if (c.cell && c.cul < 2) {
                const RowInfo& ri = c.row(c.cn);
                gv = gamma_mt((double)expf(la), (uint32_t)c.cul, (uint32_t)(t + off), (uint32_t)ri.fold, ri.stream, a.k0,
                              a.k1);
            }
            const double gy = __shfl(gv, base + 1);
            float xv = 0.f;
            {
#pragma clang fp contract(off)
                const float sb = (float)(gv / (gv + gy));
                xv = 2.0f * sb - 1.0f;
            }
            x = __shfl(xv, base);
        } else {
            x = mol_sample_row16(la, lb, s.pg, c.cul, c.l);
            s.pg = s.pgn;
        }
        if (c.w == 0 && c.cell && c.cul == 0) {
            int nn = c.cn;
            asm volatile("" : "+v"(nn));
            bst(x, mk_rsrc(a.samples), (unsigned)(out_row(nn) * a.ld) * 4u, (unsigned)(t + off) * 4u);
        }
    }
    return x;
}
// ---- GRU1 of step t + 1 for the slot's units -> x1, h1 ---------------------------------------
//   gi = W_ih1 (cI + w0 x) + b_ih1 = P1 + v x ; x1 = (cI + w0 x) + h1
//   (returns the cell's x1: with h1 the chunk state a time-sliced launch saves at its end)
template <int NT>
__device__ __forceinline__ float gen_gru1_pub(const GenCell<NT>& c, GenState& s, float x, const float4& pp, float g1r,
                                              float g1z, float g1n, unsigned seq) {
    float x1 = 0.f;
    if (c.gcell) {
        s.h1r = p_gru(fmaf(s.vr, x, pp.x), fmaf(s.vz, x, pp.y), fmaf(s.vn, x, pp.z), g1r, g1z, g1n, s.h1r);
        x1 = p_add(fmaf(s.w0c, x, pp.w), s.h1r);
    }
    c.pub(GX_X1, GS_X, c.o_px, x1, seq + 1u);
    c.pub(GX_H1, GS_X, c.o_px, s.h1r, seq + 1u);
    return x1;
}
// the step's end: progress for the host's callback, and its abort (seen at the next step's check)
template <int NT>
__device__ __forceinline__ void gen_step_end(const PersistGenArgs& a, const GenCell<NT>& c, int t) {
    if (c.w == 0 && threadIdx.x == 0) {
        if (c.g == 0) p_progress(a.progress, a.prog_base, t);
        if (p_abort(a.ctl, a.progress, t)) c.lds[GenLds<NT>::FAIL] = 1.f;
    }
}

// Poll the lane's NP B-operand packets (1 KiB apart) until none holds the sentinel; lanes
// without a packet (rows >= R) load from kNoOff, which reads 0. Bounded: records the first
// timeout's site like the other wide kernels.
template <int NP>
__device__ __forceinline__ bool g_poll(rsrc_t xr, unsigned voff, unsigned so, bool valid, u4v (&cc)[2],
                                       unsigned* ctl, unsigned where, unsigned step) {
    const unsigned t0 = p_now();
    unsigned nsp = 0;
    while (true) {
        unsigned vo = valid ? voff : kNoOff;
        asm volatile("" : "+v"(vo));
        cc[0] = __builtin_amdgcn_raw_buffer_load_b128(xr, vo, so, kCpNT);
        if constexpr (NP == 2) cc[1] = __builtin_amdgcn_raw_buffer_load_b128(xr, vo + 1024u, so, kCpNT);
        bool ok = packet_ready(cc[0]);
        if constexpr (NP == 2) ok &= packet_ready(cc[1]);
        if (__all((int)ok)) return true;
        if ((++nsp & 63) == 0 && (ld_sc1_u(ctl + PC_ERR) || p_now() - t0 > kSpinTicks)) {
            spin_give_up(ctl, where, step, true);
            return false;
        }
    }
}
// g_poll over both tiles: the lane's NP packets of tile 0 and of tile 1 (kTile1B behind) in one
// pass, until none holds the sentinel; bounded and recorded exactly as g_poll
template <int NP>
__device__ __forceinline__ bool g_poll2(rsrc_t xr, unsigned voff, unsigned so, bool valid0, bool valid1,
                                        u4v (&c0)[2], u4v (&c1)[2], unsigned* ctl, unsigned where, unsigned step) {
    const unsigned t0 = p_now();
    unsigned nsp = 0;
    while (true) {
        unsigned vo0 = valid0 ? voff : kNoOff, vo1 = valid1 ? voff : kNoOff;
        asm volatile("" : "+v"(vo0), "+v"(vo1));
        c0[0] = __builtin_amdgcn_raw_buffer_load_b128(xr, vo0, so, kCpNT);
        if constexpr (NP == 2) c0[1] = __builtin_amdgcn_raw_buffer_load_b128(xr, vo0 + 1024u, so, kCpNT);
        c1[0] = __builtin_amdgcn_raw_buffer_load_b128(xr, vo1, so + kTile1B, kCpNT);
        if constexpr (NP == 2) c1[1] = __builtin_amdgcn_raw_buffer_load_b128(xr, vo1 + 1024u, so + kTile1B, kCpNT);
        bool ok = packet_ready(c0[0]);
        ok &= packet_ready(c1[0]);
        if constexpr (NP == 2) {
            ok &= packet_ready(c0[1]);
            ok &= packet_ready(c1[1]);
        }
        if (__all((int)ok)) return true;
        if ((++nsp & 63) == 0 && (ld_sc1_u(ctl + PC_ERR) || p_now() - t0 > kSpinTicks)) {
            spin_give_up(ctl, where, step, true);
            return false;
        }
    }
}

// ---- ring instances: the slot's per-step operands, formed into the one-slot LDS arrays; produced
// and consumed by the same workgroup only. In two parts each, so that the 32-row instances can
// issue a step's table loads and draw its Philox words at the top of the step and form the values
// after its second barrier; the 16-row instances (and the prologue) run both parts at once
// (ring_p1_make, ring_noise_make) -------------------------------------------------------------
// P1(tau) of (row ri, unit 8 w + j) from the per-frame tables, k_p1_expand's fma chain without its
// zero tap (as kernels_persist_wide.hip p1_make): positions >= L take the zero frame at fbase
// (bias only), frames outside the utterance its zeroed guard slots; tau is clamped at the row's
// last step, as the stream read clamps it. In a time-sliced launch tau counts from the row's
// offset `off` (ri.rel0 carries it already), so the row's last step is S - 1 - off.
struct RingP1Taps {
    float4 tk, tq[4], ta;
};
__device__ __forceinline__ void ring_p1_load(const PersistGenRingArgs& a, const RowInfo& ri, int w, int j, int tau,
                                             RingP1Taps& o, int off = 0) {
    const int tc = tau < a.S - off ? tau : a.S - off - 1;
    int uu = GU * w + j;
    asm volatile("" : "+v"(uu));
    const unsigned p = (unsigned)(ri.rel0 + tc);
    const bool in = p < (unsigned)ri.L;  // else the zero tail pad: bias only (zero frame)
    const unsigned f = p / (unsigned)a.hop, sph = in ? p - f * (unsigned)a.hop : 0u;
    const unsigned s0 = in ? (unsigned)ri.fbase - 1u + f + (sph >= (unsigned)a.p1split ? 1u : 0u)
                           : (unsigned)ri.fbase;
    constexpr unsigned kRow = 4u * GH * 4u;  // bytes per frame slot
    const unsigned col = (unsigned)uu * 16u;
    o.tk = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(mk_rsrc(a.p1taps), sph * 16u, 0, 0));
    const rsrc_t qr = mk_rsrc(a.p1q);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        o.tq[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                 qr, (in ? s0 + (unsigned)k : s0) * kRow + col, 0, 0));
    o.ta = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                          mk_rsrc(a.p1a), (in ? (unsigned)ri.fbase + 1u + f : s0) * kRow + col, 0, 0));
}
__device__ __forceinline__ float4 ring_p1_finish(const RingP1Taps& o) {
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    const float kk[4] = {o.tk.x, o.tk.y, o.tk.z, o.tk.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        m.x = fmaf(kk[k], o.tq[k].x, m.x);
        m.y = fmaf(kk[k], o.tq[k].y, m.y);
        m.z = fmaf(kk[k], o.tq[k].z, m.z);
        m.w = fmaf(kk[k], o.tq[k].w, m.w);
    }
    return make_float4(p_add(m.x, o.ta.x), p_add(m.y, o.ta.y), p_add(m.z, o.ta.z), p_add(m.w, o.ta.w));
}
// The Gumbel word of (tau, row ri, class) as k_gumbel forms it (philox.h gumbel_q_of, keyed by
// class quad, absolute step, fold, stream). Thread j of a row takes class j of slot w (cpw 16,
// ntc 1) or the pair 2 j, 2 j + 1 (cpw 32, ntc 2: one Philox block for both): the Philox words of
// the thread's class (wd) and, ntc 2, of class c + 1 of the same quad (wd1; c is even)
// (a padding row repeats the last real row: drawn and never used); the absolute step of a
// time-sliced launch's row is tau + off
__device__ __forceinline__ void ring_noise_words(const PersistGenRingArgs& a, const RowInfo& ri, int w, int ntc, int j,
                                                 int tau, uint32_t& wd, uint32_t& wd1, int off = 0) {
    int c = a.cpw * w + (ntc == 2 ? 2 * j : j);
    asm volatile("" : "+v"(c));
    const U4 o = philox4x32_10((uint32_t)(c >> 2), (uint32_t)(tau + off), (uint32_t)ri.fold, ri.stream, a.k0, a.k1);
    const int q = c & 3;
    wd = q == 0 ? o.x : q == 1 ? o.y : q == 2 ? o.z : o.w;
    wd1 = q == 0 ? o.y : o.w;
}
// where thread j of row n writes its Gumbel words
template <class L>
__device__ __forceinline__ float* ring_noise_dst(float* lds, int ntc, int n, int j) {
    return lds + L::GR + n * kGrW + (ntc == 2 ? 2 * j : j);
}
template <class L>
__device__ __forceinline__ void ring_noise_make(const PersistGenRingArgs& a, float* lds, int w, int ntc, int n, int j,
                                                int tau, int off = 0) {
    uint32_t wd, wd1;
    ring_noise_words(a, reinterpret_cast<const RowInfo*>(lds + L::RI)[n], w, ntc, j, tau, wd, wd1, off);
    float* dst = ring_noise_dst<L>(lds, ntc, n, j);
    dst[0] = __uint_as_float(gumbel_q_of(wd));
    if (ntc == 2) {
        __builtin_amdgcn_sched_barrier(0);
        dst[1] = __uint_as_float(gumbel_q_of(wd1));
    }
}
template <class L>
__device__ __forceinline__ void ring_p1_make(const PersistGenRingArgs& a, float* lds, int w, int n, int j, int tau,
                                             int off = 0) {
    RingP1Taps taps;
    ring_p1_load(a, reinterpret_cast<const RowInfo*>(lds + L::RI)[n], w, j, tau, taps, off);
    reinterpret_cast<float4*>(lds + L::P1R)[n * GU + j] = ring_p1_finish(taps);
}
}  // namespace

// MODE: 0 BITS (categorical), 1 MOL, 2 BETA (geneing 'RAW'); each its own instantiation (the BETA
//       float64 gamma sampler would otherwise raise the other instances' register allocation)
// RING: P1 (every head) and the Gumbel noise (BITS) formed in-kernel into LDS instead of read from
//       the call's streams (MOL keeps its k_mol_noise stream). A ring instance takes
//       PersistGenRingArgs (the per-frame tables behind the common arguments); the stream
//       instances keep PersistGenArgs, so their code is what it was before the ring existed
// DBG: the instance that records logits for the teacher-forced gate (wrnn_set_debug_steps)
template <int MODE, bool RING, bool DBG>
__global__ __launch_bounds__(kPT, 1) void k_persist_wide_gen(
    std::conditional_t<RING, PersistGenRingArgs, PersistGenArgs> a) {
    static_assert(MODE >= 0 && MODE <= 2, "BITS, MOL or BETA");
    using L = GenLds<1>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int g, w;
    if (!gen_register<L>(a.ctl, lds, g, w)) return;
    const int tid = threadIdx.x;
    const GenCell<1> c = gen_cell<MODE, 1>(a, lds, g, w);
    const int v = c.v;
    const bool bvalid = c.bn < c.R;
    const unsigned o_cx = g_cons_x(v, c.l), o_cy = g_cons_y(v, c.l);
    float4 wq[kWgq];
    gen_load_weights(a, c, wq);
    gen_setup_lds(a, c);
    GenState s = gen_state(a, c);
    const rsrc_t fcr = mk_rsrc(a.fcond);
    // stream instances: in-step byte offsets of the cell's stream operands (the step's base is
    // uniform, 64-bit)
    [[maybe_unused]] const unsigned o_p1 = (unsigned)((c.cell ? c.cn : 0) * kPG * 4 * GH + c.cu * 4) * 4u;
    [[maybe_unused]] const unsigned o_gn = (unsigned)(c.crow * a.n_classes + a.cpw * w + c.cul) * 4u;
    // ring instances: thread i of waves 4-7 forms the P1 cell (row i / 8, unit i % 8) for i < 8 R
    // and, BITS, the noise cell (row i / 16, thread i % 16 of the row) for i < 16 R into the
    // one-slot LDS arrays
    [[maybe_unused]] auto ring_make = [&](const PersistGenRingArgs& ra, int t_noise, int t_p1) {
        const int i = tid - 256;
        if (i < GU * c.R) ring_p1_make<L>(ra, lds, w, i >> 3, i & 7, t_p1);
        if constexpr (MODE == 0)
            if (i < 16 * c.R) ring_noise_make<L>(ra, lds, w, c.ntc, i >> 4, i & 15, t_noise);
    };
    __syncthreads();
    // ring prologue: the noise of step t0 and P1(t0 + 1) (step t forms the noise of t + 1 and
    // P1(t + 2)); waves 0-3 read them after step t0's first barrier
    if constexpr (RING)
        if (v >= 4) ring_make(a, a.t0, a.t0 + 1);
    if constexpr (MODE == 1) {  // the draws of step t0 (the loop loads those of t + 1 at step t)
        gen_mol_draw(a, c, s, a.t0);
        s.pg = s.pgn;
    }
    if (v < 4) gen_pub_initial(a, c, s);
    bool fail = false;
    u4v cc[2];
    if (a.stamps && g == 0 && w == 0 && tid == 0) a.stamps[0] = p_now();
    for (int t = a.t0; t < a.t1; ++t) {
        const unsigned seq = (unsigned)t + 1u;
        // ---- per-step cell operands: fc1 conditioning of frame(t), the noise of step t, P1 of
        // step t + 1 (clamped at the last step, where its GRU1 goes unused) ------------------
        const float pc = gen_fc1_cond(a, c, fcr, t);
        [[maybe_unused]] float pn[2] = {0.f, 0.f};
        float4 pp = make_float4(0.f, 0.f, 0.f, 0.f);
        // (ring instances: pn and pp come from the LDS arrays after this step's first barrier)
        if constexpr (MODE == 0 && !RING) {
            if (c.cell) {
                const rsrc_t nr_ = mk_rsrc(a.gumbel + (size_t)t * a.B * a.n_classes);
                pn[0] = bld(nr_, o_gn, 0);
                if (c.ntc == 2) pn[1] = bld(nr_, o_gn + 64u, 0);
            }
        } else if constexpr (MODE == 1) {
            gen_mol_draw(a, c, s, t + 1);
        }
        if constexpr (!RING) {
            if (c.gcell) {
                const int tn = t + 1 < a.S ? t + 1 : t;
                pp = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                    mk_rsrc(a.P1 + ((size_t)tn * a.B + c.g0) * 4 * GH), o_p1, 0, 0));
            }
        }
        // ---- hop 1: x1 of every slot -> fc1 -> y1 -------------------------------------------
        fail |= !g_poll<2>(c.xr, o_cx, g_slot(GX_X1, GS_X, seq), bvalid, cc, a.ctl, c.wh(1), (unsigned)t);
        {
            v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) acc = mfma4(f4c(wq[4 + ks / 4], ks % 4), u4c(cc[ks >> 2], ks & 3), acc);
            c.put(L::F1, 1, 0, 0, acc);
        }
        if (fail) lds[L::FAIL] = 1.f;
        lds_barrier();
        if (lds[L::FAIL] != 0.f) return;
        if (v < 4) {
            gen_pub_y1(c, pc, seq);
            if constexpr (RING) gen_ring_read<MODE>(c, pn, pp);
        }
        // ---- in the wait for y1: h1 of every slot -> W_hh1 h1 (GRU1 at this step's end) ------
        fail |= !g_poll<2>(c.xr, o_cx, g_slot(GX_H1, GS_X, seq), bvalid, cc, a.ctl, c.wh(2), (unsigned)t);
        {
            v4f a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const float b = u4c(cc[ks >> 2], ks & 3);
                a0 = mfma4(f4c(wq[ks / 4], ks % 4), b, a0);
                a1 = mfma4(f4c(wq[2 + ks / 4], ks % 4), b, a1);
            }
            c.put(L::HH, 2, 0, 0, a0);
            c.put(L::HH, 2, 0, 1, a1);
        }
        // ---- hop 2: y1 of every slot -> fc3 -> the slot's candidate of every row ------------
        // (MOL / BETA: one tile; slots 2-31, for BETA 1-31, run it on their zero image, so every
        // slot polls y1 at every step as in BITS and the sentinel protocol of y1 is unchanged)
        fail |= !g_poll<1>(c.xr, o_cy, g_slot(GX_Y1, GS_Y, seq), bvalid, cc, a.ctl, c.wh(3), (unsigned)t);
        {
            v4f a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const float b = u4c(cc[0], ks);
                a0 = mfma4(f4c(wq[6], ks), b, a0);
                if (c.ntc == 2) a1 = mfma4(f4c(wq[7], ks), b, a1);
            }
            c.put(L::F3, 2, 0, 0, a0);
            if (c.ntc == 2) c.put(L::F3, 2, 0, 1, a1);
        }
        if (fail) lds[L::FAIL] = 1.f;
        lds_barrier();
        if (v < 4) {
            float g1r, g1z, g1n;
            gen_pub_fc3<MODE, DBG>(a, c, s, pn, t, seq);
            gen_gh1(c, g1r, g1z, g1n);
            const float x = gen_sample<MODE>(a, c, s, t, seq, fail);
            if (fail) lds[L::FAIL] = 1.f;  // seen by every wave at the next step's check
            gen_gru1_pub(c, s, x, pp, g1r, g1z, g1n, seq);
        } else if constexpr (RING) {
            // waves 4-7: the noise of step t + 1 and P1(t + 2) into the one-slot LDS arrays, while
            // waves 0-3 run the fc3 epilogue, hop 3 and GRU1 (they read the step-t values before
            // the barrier above and read the new ones after the next step's first barrier)
            ring_make(a, t + 1, t + 2);
        }
        gen_step_end(a, c, t);
    }
    if (a.stamps && g == 0 && w == 0 && tid == 0) a.stamps[1] = p_now();
}

// ---- time-sliced ring instances ----------------------------------------------
// The 16-row ring instance over a virtual-row map (PersistGenArgs::vmap): slot r of group g is the
// virtual row g + 8 r, which a.vmap maps to (physical row, step offset off). The launch runs its
// own steps t = 0 .. t1 - 1 with launch-local exchange tags (seq = t + 1); the row's step is
// t + off. a.rows is the launch's RowInfo table by virtual row with rel0 advanced by off, so the
// frame lookups (fc1 conditioning, P1) take t as it is; off enters the step clamp of P1, the Philox
// step of the noise and of the Beta draws, the MOL draw row, the column of the outputs and the
// captured logit's step. The row's x1, h1 come from its chunk state (k_persist_gen_init, or the
// launch that ran the row before) and go back there at the launch's end. A kernel of its own, so
// that the instances above keep their code; the step is theirs piece by piece (gen_*, ring_*), so a
// row's outputs are the unsliced launch's bit for bit.
template <int MODE, bool DBG>
__global__ __launch_bounds__(kPT, 1) void k_persist_wide_gen_rot(PersistGenRingArgs a) {
    static_assert(MODE >= 0 && MODE <= 2, "BITS, MOL or BETA");
    using L = GenLds<1>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int g, w;
    if (!gen_register<L>(a.ctl, lds, g, w)) return;
    const int tid = threadIdx.x;
    GenCell<1> c = gen_cell<MODE, 1>(a, lds, g, w);
    // the cell's step offset; its row (c.crow: chunk state, draw stream, captured logits) becomes
    // the physical one (gen_cell left the virtual row there: below 8 R, inside the map)
    const int2 cvm = a.vmap[c.crow];
    c.crow = cvm.x;
    const int coff = cvm.y;
    const int v = c.v;
    const bool bvalid = c.bn < c.R;
    const unsigned o_cx = g_cons_x(v, c.l), o_cy = g_cons_y(v, c.l);
    float4 wq[kWgq];
    gen_load_weights(a, c, wq);
    gen_setup_lds(a, c);
    if (tid < c.R) reinterpret_cast<int2*>(lds + L::VM)[tid] = a.vmap[c.g0 + kPG * tid];
    GenState s = gen_state(a, c);
    const rsrc_t fcr = mk_rsrc(a.fcond);
    // waves 4-7 form the rows' P1 and noise cells as in the plain ring instance, each row at its
    // own offset
    auto ring_make = [&](int t_noise, int t_p1) {
        const int i = tid - 256;
        const int2* vm = reinterpret_cast<const int2*>(lds + L::VM);
        if (i < GU * c.R) ring_p1_make<L>(a, lds, w, i >> 3, i & 7, t_p1, vm[i >> 3].y);
        if constexpr (MODE == 0)
            if (i < 16 * c.R) ring_noise_make<L>(a, lds, w, c.ntc, i >> 4, i & 15, t_noise, vm[i >> 4].y);
    };
    __syncthreads();
    // prologue: the noise of the row's first step and P1 of its second
    if (v >= 4) ring_make(0, 1);
    if constexpr (MODE == 1) {
        gen_mol_draw<1, true>(a, c, s, 0, coff);
        s.pg = s.pgn;
    }
    if (v < 4) gen_pub_initial(a, c, s);
    bool fail = false;
    u4v cc[2];
    if (a.stamps && g == 0 && w == 0 && tid == 0) a.stamps[0] = p_now();
    for (int t = 0; t < a.t1; ++t) {
        const unsigned seq = (unsigned)t + 1u;
        const float pc = gen_fc1_cond(a, c, fcr, t);
        [[maybe_unused]] float pn[2] = {0.f, 0.f};
        float4 pp = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (MODE == 1) gen_mol_draw<1, true>(a, c, s, t + 1, coff);
        // ---- hop 1: x1 of every slot -> fc1 -> y1 -------------------------------------------
        fail |= !g_poll<2>(c.xr, o_cx, g_slot(GX_X1, GS_X, seq), bvalid, cc, a.ctl, c.wh(1), (unsigned)t);
        {
            v4f acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) acc = mfma4(f4c(wq[4 + ks / 4], ks % 4), u4c(cc[ks >> 2], ks & 3), acc);
            c.put(L::F1, 1, 0, 0, acc);
        }
        if (fail) lds[L::FAIL] = 1.f;
        lds_barrier();
        if (lds[L::FAIL] != 0.f) return;
        if (v < 4) {
            gen_pub_y1(c, pc, seq);
            gen_ring_read<MODE>(c, pn, pp);
        }
        // ---- in the wait for y1: h1 of every slot -> W_hh1 h1 --------------------------------
        fail |= !g_poll<2>(c.xr, o_cx, g_slot(GX_H1, GS_X, seq), bvalid, cc, a.ctl, c.wh(2), (unsigned)t);
        {
            v4f a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const float b = u4c(cc[ks >> 2], ks & 3);
                a0 = mfma4(f4c(wq[ks / 4], ks % 4), b, a0);
                a1 = mfma4(f4c(wq[2 + ks / 4], ks % 4), b, a1);
            }
            c.put(L::HH, 2, 0, 0, a0);
            c.put(L::HH, 2, 0, 1, a1);
        }
        // ---- hop 2: y1 of every slot -> fc3 -> the slot's candidate (logits) of every row ------
        fail |= !g_poll<1>(c.xr, o_cy, g_slot(GX_Y1, GS_Y, seq), bvalid, cc, a.ctl, c.wh(3), (unsigned)t);
        {
            v4f a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const float b = u4c(cc[0], ks);
                a0 = mfma4(f4c(wq[6], ks), b, a0);
                if (c.ntc == 2) a1 = mfma4(f4c(wq[7], ks), b, a1);
            }
            c.put(L::F3, 2, 0, 0, a0);
            if (c.ntc == 2) c.put(L::F3, 2, 0, 1, a1);
        }
        if (fail) lds[L::FAIL] = 1.f;
        lds_barrier();
        if (v < 4) {
            float g1r, g1z, g1n;
            gen_pub_fc3<MODE, DBG>(a, c, s, pn, t, seq, coff);
            gen_gh1(c, g1r, g1z, g1n);
            const float x = gen_sample<MODE, 1, true>(a, c, s, t, seq, fail, coff);
            if (fail) lds[L::FAIL] = 1.f;  // seen by every wave at the next step's check
            s.x1c = gen_gru1_pub(c, s, x, pp, g1r, g1z, g1n, seq);
        } else {
            ring_make(t + 1, t + 2);  // (the row's last step: P1 clamped, its GRU1 goes unused)
        }
        gen_step_end(a, c, t);
    }
    if (a.stamps && g == 0 && w == 0 && tid == 0) a.stamps[1] = p_now();
    // x1, h1 of the launch's last GRU1 (the row's step off + t1) back into the chunk state, for the
    // launch that runs the row next. A cell reads and writes its own two words only, and the next
    // launch starts after this one has finished
    if (c.gcell && !fail && lds[L::FAIL] == 0.f) {
        float* st = a.st + (size_t)c.crow * 2 * GH;
        st[c.cu] = s.x1c;
        st[GH + c.cu] = s.h1r;
    }
}

// ---- 32-row ring instances ------------------------------------------------------------------
// Up to 32 rows per XCD group in one launch: rows 0-15 of a group are MFMA column tile 0, rows
// 16-31 column tile 1. Every wave polls both tiles' B-operand packets and runs each product for
// both tiles on the same weight registers (two independent accumulator chains); the epilogue
// cells of tile 0 lie on waves 0-3, those of tile 1 on waves 4-7, one cell per lane in the
// (cn, cul) layout of a tile. A row's arithmetic is the 16-row ring instance's: the same weight
// registers, the same K split over the 8 waves, the same fixed-order sum of the 8 partials, and
// the same step pieces (gen_*, ring_*), so its outputs are the 16-row instance's bit for bit.
// Ring form only (no stream instance).
//
// Exchange: tile 1 has its own copy of the whole per-group area (x1 / h1 / y1 parity slots and the
// candidate / logit-pair area) kTile1B bytes behind tile 0's, so the offset functions above serve
// both tiles; a group's area is 2 GX_GROUP floats. LDS: the partial buffers, the ring arrays and
// the RowInfo array are twice the 16-row kernel's (GenLds<2>).
//
// Ring work: waves 4-7 have no free tail here, so each wave set forms its own tile's next noise /
// P1 in two parts. At the top of a step, before the hop-1 poll, a thread issues the table loads of
// its P1 cell (their addresses depend only on t and the row; in flight over the whole step) and
// forms the Philox words and the first Gumbel word of its noise cell in the wait for x1. After it
// has published its fc3 candidates (logits) and before it polls the candidates of hop 3 -- in the
// flight time of that exchange -- it forms the second Gumbel word and the P1 value and writes both
// cells. The order is kept by the same two barriers: the arrays are read after a step's first
// barrier and written after its second.
template <int MODE, bool DBG>
__global__ __launch_bounds__(kPT, 1) void k_persist_wide_gen32(PersistGenRingArgs a) {
    static_assert(MODE >= 0 && MODE <= 2, "BITS, MOL or BETA");
    using L = GenLds<2>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int g, w;
    if (!gen_register<L>(a.ctl, lds, g, w)) return;
    const int tid = threadIdx.x;
    const GenCell<2> c = gen_cell<MODE, 2>(a, lds, g, w);
    const int v = c.v;
    const bool bvalid0 = c.bn < c.R, bvalid1 = kRowsW + c.bn < c.R;
    const unsigned o_cx = g_cons_x(v, c.l), o_cy = g_cons_y(v, c.l);
    float4 wq[kWgq];  // (the 16-row kernel's image and register assignment)
    gen_load_weights(a, c, wq);
    gen_setup_lds(a, c);
    GenState s = gen_state(a, c);
    const rsrc_t fcr = mk_rsrc(a.fcond);
    // thread i of a wave set forms, for its tile, the P1 cell (row i / 8, unit i % 8) and, BITS, the
    // noise cell (row i / 16, thread i % 16 of the row) of the rows below R
    const int ri_ = tid & 255;
    const int n1 = kRowsW * c.tt + (ri_ >> 3), n2 = kRowsW * c.tt + (ri_ >> 4);
    const bool p1do = n1 < c.R, nzdo = MODE == 0 && n2 < c.R;
    __syncthreads();
    // ring prologue (both parts at once): the noise of step t0 and P1(t0 + 1), read after step t0's
    // first barrier
    if (p1do) ring_p1_make<L>(a, lds, w, n1, ri_ & 7, a.t0 + 1);
    if constexpr (MODE == 0)
        if (nzdo) ring_noise_make<L>(a, lds, w, c.ntc, n2, ri_ & 15, a.t0);
    if constexpr (MODE == 1) {
        gen_mol_draw(a, c, s, a.t0);
        s.pg = s.pgn;
    }
    gen_pub_initial(a, c, s);
    bool fail = false;
    u4v c0[2], c1[2];
    if (a.stamps && g == 0 && w == 0 && tid == 0) a.stamps[0] = p_now();
    for (int t = a.t0; t < a.t1; ++t) {
        const unsigned seq = (unsigned)t + 1u;
        const float pc = gen_fc1_cond(a, c, fcr, t);
        [[maybe_unused]] float pn[2] = {0.f, 0.f};
        float4 pp = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (MODE == 1) gen_mol_draw(a, c, s, t + 1);
        // the thread's ring cells of the next step, first part: the table loads of P1(t + 2) are in
        // flight over the whole step, the Philox words of step t + 1 and the first Gumbel word are
        // formed in the wait for x1; the values go to LDS after the second barrier
        RingP1Taps pt;
        [[maybe_unused]] uint32_t nw0 = 0, nw1 = 0, ng0 = 0;
        if (p1do) ring_p1_load(a, c.row(n1), w, ri_ & 7, t + 2, pt);
        if constexpr (MODE == 0) {
            if (nzdo) {
                ring_noise_words(a, c.row(n2), w, c.ntc, ri_ & 15, t + 1, nw0, nw1);
                ng0 = gumbel_q_of(nw0);
            }
            asm volatile("" : "+v"(ng0), "+v"(nw1));
        }
        // ---- hop 1: x1 of every slot, both tiles -> fc1 -> y1 --------------------------------
        fail |= !g_poll2<2>(c.xr, o_cx, g_slot(GX_X1, GS_X, seq), bvalid0, bvalid1, c0, c1, a.ctl, c.wh(1), (unsigned)t);
        {
            v4f e0 = {0.f, 0.f, 0.f, 0.f}, e1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const float wa = f4c(wq[4 + ks / 4], ks % 4);
                e0 = mfma4(wa, u4c(c0[ks >> 2], ks & 3), e0);
                e1 = mfma4(wa, u4c(c1[ks >> 2], ks & 3), e1);
            }
            c.put(L::F1, 1, 0, 0, e0);
            c.put(L::F1, 1, 1, 0, e1);
        }
        if (fail) lds[L::FAIL] = 1.f;
        lds_barrier();
        if (lds[L::FAIL] != 0.f) return;
        gen_pub_y1(c, pc, seq);
        gen_ring_read<MODE>(c, pn, pp);
        // ---- in the wait for y1: h1 of every slot -> W_hh1 h1 ---------------------------------
        fail |= !g_poll2<2>(c.xr, o_cx, g_slot(GX_H1, GS_X, seq), bvalid0, bvalid1, c0, c1, a.ctl, c.wh(2), (unsigned)t);
        {
            v4f a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
            v4f b0 = {0.f, 0.f, 0.f, 0.f}, b1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const float x0 = u4c(c0[ks >> 2], ks & 3), x1 = u4c(c1[ks >> 2], ks & 3);
                const float wa = f4c(wq[ks / 4], ks % 4), wb = f4c(wq[2 + ks / 4], ks % 4);
                a0 = mfma4(wa, x0, a0);
                b0 = mfma4(wa, x1, b0);
                a1 = mfma4(wb, x0, a1);
                b1 = mfma4(wb, x1, b1);
            }
            c.put(L::HH, 2, 0, 0, a0);
            c.put(L::HH, 2, 0, 1, a1);
            c.put(L::HH, 2, 1, 0, b0);
            c.put(L::HH, 2, 1, 1, b1);
        }
        // ---- hop 2: y1 of every slot -> fc3 -> the slot's candidate of every row ------------
        fail |= !g_poll2<1>(c.xr, o_cy, g_slot(GX_Y1, GS_Y, seq), bvalid0, bvalid1, c0, c1, a.ctl, c.wh(3), (unsigned)t);
        {
            v4f a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
            v4f b0 = {0.f, 0.f, 0.f, 0.f}, b1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const float x0 = u4c(c0[0], ks), x1 = u4c(c1[0], ks);
                a0 = mfma4(f4c(wq[6], ks), x0, a0);
                b0 = mfma4(f4c(wq[6], ks), x1, b0);
                if (c.ntc == 2) {
                    a1 = mfma4(f4c(wq[7], ks), x0, a1);
                    b1 = mfma4(f4c(wq[7], ks), x1, b1);
                }
            }
            c.put(L::F3, 2, 0, 0, a0);
            c.put(L::F3, 2, 1, 0, b0);
            if (c.ntc == 2) {
                c.put(L::F3, 2, 0, 1, a1);
                c.put(L::F3, 2, 1, 1, b1);
            }
        }
        if (fail) lds[L::FAIL] = 1.f;
        lds_barrier();
        {
            float g1r, g1z, g1n;
            gen_pub_fc3<MODE, DBG>(a, c, s, pn, t, seq);
            gen_gh1(c, g1r, g1z, g1n);
            // second part, while the candidates travel: the tile's noise of step t + 1 and P1(t + 2)
            if constexpr (MODE == 0) {
                if (nzdo) {
                    float* dst = ring_noise_dst<L>(lds, c.ntc, n2, ri_ & 15);
                    dst[0] = __uint_as_float(ng0);
                    if (c.ntc == 2) dst[1] = __uint_as_float(gumbel_q_of(nw1));
                }
            }
            if (p1do) reinterpret_cast<float4*>(lds + L::P1R)[n1 * GU + (ri_ & 7)] = ring_p1_finish(pt);
            const float x = gen_sample<MODE>(a, c, s, t, seq, fail);
            if (fail) lds[L::FAIL] = 1.f;  // seen by every wave at the next step's check
            gen_gru1_pub(c, s, x, pp, g1r, g1z, g1n, seq);
        }
        gen_step_end(a, c, t);
    }
    if (a.stamps && g == 0 && w == 0 && tid == 0) a.stamps[1] = p_now();
}

// launch-side helpers --------------------------------------------------------------------
namespace {
// at least 96 KB so that no CU can take two workgroups of this (register-light) kernel: every
// group must span 32 CUs
constexpr size_t gen_lds_bytes(int floats) {
    const size_t need = (size_t)floats * sizeof(float);
    return need > 96 * 1024 ? need : 96 * 1024;
}
// before every launch: the vector slots to the sentinel, the candidate / logit areas (step tags)
// to 0, over n16 16-byte units (every tile copy is GX_GROUP floats)
__global__ __launch_bounds__(256) void k_wide_gen_xbuf_reset(uint4* x, size_t n16) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n16) return;
    const unsigned f = (unsigned)((i * 4) % GX_GROUP);
    x[i] = f >= (unsigned)GX_D ? make_uint4(0u, 0u, 0u, 0u) : make_uint4(kSent, kSent, kSent, kSent);
}
hipError_t gen_reset_xbuf(float* xbuf, size_t floats, hipStream_t s) {
    const unsigned n = (unsigned)(floats / 4);
    k_wide_gen_xbuf_reset<<<(n + 255) / 256, 256, 0, s>>>(reinterpret_cast<uint4*>(xbuf), floats / 4);
    return hipGetLastError();
}

// The four kernel families, instance <MODE, DBG> of each, and the one (mode x DBG) dispatch:
// f(instance) for the family's instance of (mode 0 .. 2, dbg), the kernel as decltype(k)::value
struct Gen16Stream {
    using Args = PersistGenArgs;
    template <int MODE, bool DBG>
    static constexpr auto k = k_persist_wide_gen<MODE, false, DBG>;
};
struct Gen16Ring {
    using Args = PersistGenRingArgs;
    template <int MODE, bool DBG>
    static constexpr auto k = k_persist_wide_gen<MODE, true, DBG>;
};
struct Gen32Ring {
    using Args = PersistGenRingArgs;
    template <int MODE, bool DBG>
    static constexpr auto k = k_persist_wide_gen32<MODE, DBG>;
};
struct Gen16Rot {
    using Args = PersistGenRingArgs;
    template <int MODE, bool DBG>
    static constexpr auto k = k_persist_wide_gen_rot<MODE, DBG>;
};
template <class Fam, int MODE, bool DBG>
using GenInst = std::integral_constant<void (*)(typename Fam::Args), Fam::template k<MODE, DBG>>;
template <class Fam, class F>
auto gen_dispatch(int mode, bool dbg, F&& f) {
    if (mode == 2) return dbg ? f(GenInst<Fam, 2, true>{}) : f(GenInst<Fam, 2, false>{});
    if (mode == 1) return dbg ? f(GenInst<Fam, 1, true>{}) : f(GenInst<Fam, 1, false>{});
    return dbg ? f(GenInst<Fam, 0, true>{}) : f(GenInst<Fam, 0, false>{});
}
// scratch bytes of one instance (-1: no such mode, or the query failed)
template <class Fam>
int gen_scratch_of(int mode, bool dbg) {
    if (mode < 0 || mode > 2) return -1;
    return gen_dispatch<Fam>(mode, dbg, [](auto k) {
        hipFuncAttributes fa;
        const void* fn = reinterpret_cast<const void*>(decltype(k)::value);
        return hipFuncGetAttributes(&fa, fn) == hipSuccess ? (int)fa.localSizeBytes : -1;
    });
}
// the larger scratch of a mode's production and DBG instance: a constant of the build, read from
// the code objects once per mode
template <class Fam>
int gen_scratch_max(int mode) {
    if (mode < 0 || mode > 2) return -1;
    static int cached[3] = {-2, -2, -2};  // -2: not read yet
    if (cached[mode] == -2) {
        const int p = gen_scratch_of<Fam>(mode, false), d = gen_scratch_of<Fam>(mode, true);
        if (p < 0 || d < 0) return -1;
        cached[mode] = p > d ? p : d;
    }
    return cached[mode];
}
// whole launches (t0 = 0: x1, h1 of k_persist_gen_init) of BITS rows with 512 or 1024 classes
// (1 or 2 fc3 tiles of 16 per slot), of MOL rows (30 logits; the draws come from the k_mol_noise
// stream) or of BETA rows (2): one tile in slots 0 and 1. rot: a time-sliced launch instead (its
// virtual-row map, t1 <= S steps from every row's chunk state)
bool gen_args_ok(const PersistGenArgs& a, int max_rows, bool rot = false) {
    if (a.rb < 0 || a.nr < 1 || a.nr > max_rows || a.rb + kPG * a.nr > a.B || a.t0 != 0 || a.wwide == nullptr)
        return false;
    // (a time-sliced launch indexes its map and its RowInfo table by virtual row g + 8 r: both hold
    // 8 nr entries, so the launch starts at row 0)
    if (rot ? a.vmap == nullptr || a.rb != 0 || a.t1 < 1 || a.t1 > a.S || a.st == nullptr
            : a.vmap != nullptr || a.t1 != a.S)
        return false;
    if (a.mode == 1) return a.cpw == 16 && a.n_classes == 30 && a.gumbel != nullptr;
    if (a.mode == 2) return a.cpw == 16 && a.n_classes == 2;
    return a.mode == 0 && (a.n_classes == 512 || a.n_classes == 1024) && a.cpw * kPM == a.n_classes;
}
// ring launches form P1 from the per-frame tables and read no stream, so the tables must all be there
bool gen_ring_args_ok(const PersistGenRingArgs& a) {
    return a.p1q && a.p1a && a.p1taps && a.hop > 0 && a.p1split >= 0 && a.mode >= 0 && a.mode <= 2;
}
template <class Fam>
hipError_t gen_launch(const typename Fam::Args& a, int max_rows, size_t lds, hipStream_t s) {
    if (!gen_args_ok(a, max_rows, std::is_same_v<Fam, Gen16Rot>)) return hipErrorInvalidValue;
    return gen_dispatch<Fam>(a.mode, a.dbg.out != nullptr,
                             [&](auto k) { return persist_launch<decltype(k)::value>(lds, a, s); });
}
}  // namespace

size_t persist_wide_gen_lds_bytes() { return gen_lds_bytes(GenLds<1>::TOTAL_RING); }  // (stream instances use TOTAL of it)
size_t persist_wide_gen_xbuf_floats() { return (size_t)kPG * GX_GROUP; }
size_t persist_wide_gen_wreg_floats() { return (size_t)kPM * 8 * kWgq * 64 * 4; }
hipError_t persist_wide_gen_reset_xbuf(float* xbuf, hipStream_t s) {
    return gen_reset_xbuf(xbuf, persist_wide_gen_xbuf_floats(), s);
}
// scratch bytes of the mode's stream instances (0 BITS, 1 MOL, 2 BETA): the larger of production
// and DBG (BITS: the production instance, as the planner has always read it)
int persist_wide_gen_scratch(int mode) {
    return mode == 0 ? gen_scratch_of<Gen16Stream>(0, false) : gen_scratch_max<Gen16Stream>(mode);
}
// ... and of its ring instances (the larger of production and DBG): a ring launch needs 0
int persist_wide_gen_ring_scratch(int mode) { return gen_scratch_max<Gen16Ring>(mode); }
hipError_t launch_persist_wide_gen(const PersistGenArgs& a, hipStream_t s) {
    return gen_launch<Gen16Stream>(a, kPWideRows, persist_wide_gen_lds_bytes(), s);
}
// ring launch: the instances must run without scratch
hipError_t launch_persist_wide_gen_ring(const PersistGenRingArgs& a, hipStream_t s) {
    if (!gen_ring_args_ok(a) || persist_wide_gen_ring_scratch(a.mode) != 0) return hipErrorInvalidValue;
    return gen_launch<Gen16Ring>(a, kPWideRows, persist_wide_gen_lds_bytes(), s);
}

// ---- time-sliced ring instances: launch side -----------------------------------------------
// scratch bytes of the mode's time-sliced instances (the larger of production and DBG); -1: none
int persist_wide_gen_rot_scratch(int mode) { return gen_scratch_max<Gen16Rot>(mode); }
// the rule of the 16-row ring instances: no scratch; Beta at most its 16-byte frame
bool persist_wide_gen_rot_usable(int mode) {
    const int sc = persist_wide_gen_rot_scratch(mode);
    return sc >= 0 && sc <= (mode == 2 ? 16 : 0);
}
// a launch of t1 <= S steps over the rows of a.vmap (a.rows: the launch's table by virtual row).
// The MOL instance addresses the whole draw stream [S][B][kMolNoise] with a 32-bit offset
hipError_t launch_persist_wide_gen_rot(const PersistGenRingArgs& a, hipStream_t s) {
    if (!gen_ring_args_ok(a) || !persist_wide_gen_rot_usable(a.mode)) return hipErrorInvalidValue;
    if (a.mode == 1 && !((double)a.S * a.B * kMolNoise * 4.0 < 2147483648.0)) return hipErrorInvalidValue;
    return gen_launch<Gen16Rot>(a, kPWideRows, persist_wide_gen_lds_bytes(), s);
}

// ---- 32-row ring instances: launch side ---------------------------------------------------
size_t persist_wide_gen32_lds_bytes() { return gen_lds_bytes(GenLds<2>::TOTAL_RING); }
size_t persist_wide_gen32_xbuf_floats() { return (size_t)kPG * GX_GROUP32; }
// (both tile copies of every group)
hipError_t persist_wide_gen32_reset_xbuf(float* xbuf, hipStream_t s) {
    return gen_reset_xbuf(xbuf, persist_wide_gen32_xbuf_floats(), s);
}
// scratch bytes of the mode's 32-row instances (the larger of production and DBG); -1: no such instance
int persist_wide_gen32_scratch(int mode) { return gen_scratch_max<Gen32Ring>(mode); }
// the scratch a 32-row launch of the mode may carry: none; Beta at most the 16-byte frame its
// other instances are accepted with
bool persist_wide_gen32_usable(int mode) {
    const int sc = persist_wide_gen32_scratch(mode);
    return sc >= 0 && sc <= (mode == 2 ? 16 : 0);
}
// whole launches of up to 32 rows per group (t0 = 0), heads as launch_persist_wide_gen_ring
hipError_t launch_persist_wide_gen32_ring(const PersistGenRingArgs& a, hipStream_t s) {
    if (!gen_ring_args_ok(a) || !persist_wide_gen32_usable(a.mode)) return hipErrorInvalidValue;
    return gen_launch<Gen32Ring>(a, kRows32, persist_wide_gen32_lds_bytes(), s);
}

// Exhaustive host check of the exchange layout (as wide_rr_layout_check): for every row count,
// the producer packets of x1 / h1 (32 slots x R rows x 2 unit quads) and of y1 (32 slots x R
// rows x 1 quad) coincide one to one with the consumer packets (8 waves x 64 lanes x 2 or 1
// packets, lanes of rows >= R off) with matching (row, unit quad), inside the slot; every parity
// slot inside its vector's area and the areas disjoint; the no-packet offset outside every
// buffer; the candidate pairs a lane polls aligned and inside their area. Returns the violations.
int wide_gen_layout_check(int R) {
    if (R < 1 || R > kRowsW) return -1;
    int bad = 0;
    for (int kind = 0; kind < 2; ++kind) {  // 0: x1 / h1 (256 units), 1: y1 (128 units)
        const int sz = kind ? GS_Y : GS_X, upw = kind ? GO : GU, np = kind ? 1 : 2;
        std::vector<int> owner(sz / 4, -1);
        int published = 0;
        for (int w = 0; w < kPM; ++w)
            for (int cn = 0; cn < R; ++cn)
                for (int cul = 0; cul < upw; cul += 4) {
                    const int u = upw * w + cul;
                    const unsigned o = kind ? g_prod_y(u, cn) : g_prod_x(u, cn);
                    if (o % 16 || o + 16 > (unsigned)sz * 4u) { ++bad; continue; }
                    if (owner[o / 16] >= 0) ++bad;
                    owner[o / 16] = u * kRowsW + cn;
                    ++published;
                }
        int matched = 0;
        for (int v = 0; v < 8; ++v)
            for (int l = 0; l < 64; ++l) {
                if ((l & 15) >= R) continue;
                for (int p = 0; p < np; ++p) {
                    const unsigned o = (kind ? g_cons_y(v, l) : g_cons_x(v, l)) + 1024u * (unsigned)p;
                    if (o % 16 || o + 16 > (unsigned)sz * 4u) { ++bad; continue; }
                    const int ow = owner[o / 16];
                    if (ow < 0) { ++bad; continue; }
                    const int want_u = kind ? 16 * v + 4 * (l >> 4) : 32 * v + 8 * (l >> 4) + 4 * p;
                    if (ow % kRowsW != (l & 15) || ow / kRowsW != want_u) ++bad;
                    ++matched;
                }
            }
        if (matched != published) ++bad;
    }
    const int bufs[3] = {GX_X1, GX_H1, GX_Y1}, szs[3] = {GS_X, GS_X, GS_Y}, ends[3] = {GX_H1, GX_Y1, GX_D};
    for (int b = 0; b < 3; ++b)
        for (unsigned sq = 0; sq < 2; ++sq) {
            const unsigned s0 = g_slot(bufs[b], szs[b], sq);
            if (s0 < (unsigned)bufs[b] * 4u || s0 + (unsigned)szs[b] * 4u > (unsigned)ends[b] * 4u) ++bad;
            if ((unsigned long long)kNoOff + s0 + 1024ull <= 0x7fffffffull) ++bad;
        }
    if ((unsigned long long)kNoOff + (unsigned)GX_D * 4u <= 0x7fffffffull) ++bad;
    for (int n = 0; n < R; ++n)
        for (int c = 0; c < 16; ++c)
            if (g_cand(n, 2 * c) % 16 || g_cand(n, 2 * c) + 16 > (unsigned)(kRowsW * kPM * 2) * 4u ||
                g_cand(n, 2 * c + 1) != g_cand(n, 2 * c) + 8)
                ++bad;
    return bad;
}

// Host check of the MOL / BETA logit pairs (g_logit, n_logits 30 or 2) for a group of R rows:
// every (row, logit) pair is 8-byte aligned inside the area at GX_D, written by exactly one lane
// of the fc3 epilogue of exactly one slot (slot w < 2, lane cul: logit 16 w + cul < n_logits) and
// read, in every slot, by exactly one hop-3 lane of the row (lane cul: logits cul and 16 + cul)
// that expects that (row, logit); no two pairs overlap; the area lies after the vector slots,
// inside the group's exchange area, in the part the reset zeroes; the no-logit offset fails the
// range check. Returns the violations (-1: bad arguments).
int wide_gen_mol_layout_check(int R, int n_logits) {
    if (R < 1 || R > kRowsW || (n_logits != 30 && n_logits != 2)) return -1;
    int bad = 0;
    const int area = kRowsW * kPM * 2;  // floats
    const int np = area / 2;
    std::vector<int> wr(np, 0), id(np, -1);
    for (int w = 0; w < kPM; ++w)
        for (int cn = 0; cn < R; ++cn)
            for (int cul = 0; cul < 16; ++cul) {
                const int k = 16 * w + cul;
                if (w >= 2 || k >= n_logits) continue;  // (the epilogue's o_lp)
                const unsigned o = g_logit(cn, k);
                if (o % 8 || o + 8 > (unsigned)area * 4u) { ++bad; continue; }
                ++wr[o / 8];
                id[o / 8] = cn * kGenLogitsMax + k;
            }
    for (int w = 0; w < kPM; ++w) {  // the readers of slot w
        std::vector<int> rd(np, 0);
        for (int cn = 0; cn < R; ++cn)
            for (int cul = 0; cul < 16; ++cul)
                for (int k = cul; k < n_logits && k < 32; k += 16) {
                    const unsigned o = g_logit(cn, k);
                    if (o % 8 || o + 8 > (unsigned)area * 4u) { ++bad; continue; }
                    ++rd[o / 8];
                    if (id[o / 8] != cn * kGenLogitsMax + k) ++bad;  // the reader expects another (row, logit)
                }
        for (int i = 0; i < np; ++i)
            if (rd[i] > 1 || rd[i] != wr[i]) ++bad;
    }
    int pairs = 0;
    for (int i = 0; i < np; ++i) {
        if (wr[i] > 1) ++bad;
        pairs += wr[i];
    }
    if (pairs != R * n_logits) ++bad;
    // disjoint from the vector slots, inside the group's area, where the reset writes zeros
    const int bufs[3] = {GX_X1, GX_H1, GX_Y1}, szs[3] = {GS_X, GS_X, GS_Y};
    for (int b = 0; b < 3; ++b)
        for (unsigned sq = 0; sq < 2; ++sq)
            if (g_slot(bufs[b], szs[b], sq) + (unsigned)szs[b] * 4u > (unsigned)GX_D * 4u) ++bad;
    if (GX_D + area > GX_GROUP || GX_D % 2) ++bad;
    if ((unsigned long long)kNoOff + (unsigned long long)GX_D * 4ull + 8ull <= 0x7fffffffull) ++bad;
    return bad;
}

// The 32-row instances' exchange layout for a group of R rows (1 .. 32): each tile's own layout by
// the check above, then, with the kernel's own row -> (tile, column) mapping and absolute byte
// offsets inside the group's area of 2 GX_GROUP floats, every producer packet of x1 / h1 / y1 (both
// parity slots) meets exactly one consumer packet of the same (row, unit quad) and lies inside its
// tile's copy, every candidate couple a lane polls lies in its tile's candidate area, the two
// copies are disjoint, and the no-packet offset stays outside the buffer behind tile 1's offsets.
int wide_gen32_layout_check(int R) {
    if (R < 1 || R > kRows32) return -1;
    int bad = wide_gen_layout_check(R < kRowsW ? R : kRowsW);
    if (R > kRowsW) bad += wide_gen_layout_check(R - kRowsW);
    const unsigned area = (unsigned)GX_GROUP32 * 4u;
    const int bufs[3] = {GX_X1, GX_H1, GX_Y1}, szs[3] = {GS_X, GS_X, GS_Y};
    for (int b = 0; b < 3; ++b)
        for (unsigned sq = 0; sq < 2; ++sq) {
            const bool y = b == 2;
            const int upw = y ? GO : GU, np = y ? 1 : 2;
            std::vector<int> owner(area / 16, -1);
            int published = 0, matched = 0;
            for (int w = 0; w < kPM; ++w)
                for (int cn = 0; cn < R; ++cn)
                    for (int cul = 0; cul < upw; cul += 4) {
                        const int tile = cn >> 4, cnl = cn & 15, u = upw * w + cul;
                        const unsigned lo = (unsigned)tile * kTile1B;
                        const unsigned o = lo + g_slot(bufs[b], szs[b], sq) + (y ? g_prod_y(u, cnl) : g_prod_x(u, cnl));
                        if (o % 16 || o < lo || o + 16 > lo + (unsigned)GX_D * 4u || o + 16 > area) { ++bad; continue; }
                        if (owner[o / 16] >= 0) ++bad;
                        owner[o / 16] = u * kRows32 + cn;
                        ++published;
                    }
            for (int tile = 0; tile < 2; ++tile)
                for (int v = 0; v < 8; ++v)
                    for (int l = 0; l < 64; ++l) {
                        const int cn = kRowsW * tile + (l & 15);
                        if (cn >= R) continue;
                        for (int p = 0; p < np; ++p) {
                            const unsigned o = (unsigned)tile * kTile1B + g_slot(bufs[b], szs[b], sq) +
                                               (y ? g_cons_y(v, l) : g_cons_x(v, l)) + 1024u * (unsigned)p;
                            if (o % 16 || o + 16 > area) { ++bad; continue; }
                            const int ow = owner[o / 16];
                            const int want_u = y ? 16 * v + 4 * (l >> 4) : 32 * v + 8 * (l >> 4) + 4 * p;
                            if (ow != want_u * kRows32 + cn) ++bad;
                            ++matched;
                        }
                    }
            if (matched != published) ++bad;
            if ((unsigned long long)kNoOff + g_slot(bufs[b], szs[b], sq) + kTile1B + 1024ull <= 0x7fffffffull) ++bad;
        }
    for (int cn = 0; cn < R; ++cn)
        for (int c = 0; c < 16; ++c) {
            const unsigned lo = (unsigned)(cn >> 4) * kTile1B + (unsigned)GX_D * 4u;
            const unsigned o = lo + g_cand(cn & 15, 2 * c);
            if (o % 16 || o + 16 > lo + (unsigned)(kRowsW * kPM * 2) * 4u || o + 16 > (unsigned)(cn >> 4) * kTile1B + kTile1B)
                ++bad;
        }
    if ((unsigned)GX_D * 4u + (unsigned)(kRowsW * kPM * 2) * 4u > kTile1B || 2u * kTile1B != area) ++bad;  // copies disjoint
    if ((size_t)kPG * GX_GROUP32 != persist_wide_gen32_xbuf_floats()) ++bad;
    if ((unsigned long long)kNoOff + (unsigned)GX_D * 4u + kTile1B <= 0x7fffffffull) ++bad;
    return bad;
}

// ... and the MOL / BETA logit pairs of both tiles: each tile's pairs by the check above; tile 1's
// area lies behind tile 0's whole copy, inside the group's area, in the part the reset zeroes
int wide_gen32_mol_layout_check(int R, int n_logits) {
    if (R < 1 || R > kRows32 || (n_logits != 30 && n_logits != 2)) return -1;
    int bad = wide_gen_mol_layout_check(R < kRowsW ? R : kRowsW, n_logits);
    if (R > kRowsW) bad += wide_gen_mol_layout_check(R - kRowsW, n_logits);
    const unsigned pairs = (unsigned)(kRowsW * kPM * 2) * 4u;  // bytes of a tile's pair area
    for (int cn = 0; cn < R; ++cn)
        for (int k = 0; k < n_logits; ++k) {
            const unsigned lo = (unsigned)(cn >> 4) * kTile1B + (unsigned)GX_D * 4u;
            const unsigned o = lo + g_logit(cn & 15, k);
            if (o % 8 || o + 8 > lo + pairs || o + 8 > (unsigned)GX_GROUP32 * 4u) ++bad;
            // (the reset zeroes floats f of a copy with f % GX_GROUP >= GX_D)
            if ((o / 4u) % (unsigned)GX_GROUP < (unsigned)GX_D) ++bad;
        }
    if ((unsigned)GX_D * 4u + pairs > kTile1B) ++bad;  // tile 0's pairs end before tile 1's copy
    if ((unsigned long long)kNoOff + (unsigned long long)GX_D * 4ull + kTile1B + 8ull <= 0x7fffffffull) ++bad;
    return bad;
}

}  // namespace wrnn
