// Persistent fatchord recurrence for WIDE row batches of a PRUNED model (the "persist-wide-sp"
// launch kind): the block-sparse twin of k_persist_wide (kernels_persist_wide.hip). Up to 16 fold
// rows per XCD group, RAW categorical with 512 or 1024 classes.
//
// Reference: the step body of vocoder/models/fatchord_version.py:192-236 on weights the Pruner
// left with zero 1 x 4 blocks (vocoder/pruner.py:60-88), which the reference's native backend
// skips (CompMatrix::operator*, vocoder/libwavernn/runtimeracer_version/src/wavernn.cpp:162-184).
//
// Kept from k_persist_wide, unchanged: the group registration, the exchange area and packet
// protocol of wide_layout.h (sentinel slots, pub / w_poll, five hops E, A, B, C, D), the
// distributed GRU1, the epilogue cells on waves 0-3 with p_gru / p_add, the exact candidate key
// and the hop-D decision, the in-kernel P1 and noise rings, RowInfo and the vmap of time-sliced
// launches, chunk state, the abort and timeout paths, the phase stamps, the DBG logit capture.
//
// Replaced: the products. MFMA cannot skip the blocks (a 16-unit M tile drops a k-step only when
// all 16 units' blocks are zero), so they are VALU products over activations gathered from LDS:
//  * The slot's live blocks sit in LDS as one list per (product set, output row): float4 values
//    with their column-block index, by ascending column (sparse_wide_pack.h; 13 sets x 16 rows).
//  * A hop's vector still arrives as B-operand packets in registers, where the sentinel check
//    happens (w_poll). Every wave then writes its K-eighth to an LDS stage X[row][unit] (row
//    stride 516 floats: the 16 rows of one column block fall on 16 distinct bank quads), and after
//    a barrier the products gather from it.
//  * Lanes are (row, unit) cells: thread tid of waves 0-3 is the epilogue cell (row tid / 16, unit
//    16 w + tid % 16) and forms the critical products of its own cell (W_ih2 x1, fc1 x2, fc2 y1,
//    fc3 y2) whole, in registers -- no partial sums, no second barrier; thread 256 + tid of waves
//    4-7 forms the off-path products of the same cell (W_hh1 h1, W_hh2 h2) and hands the six sums
//    over in LDS (G). The 16 lanes of a unit read the same weight block (a broadcast). (Measured:
//    those two products are on the critical path -- all eight waves write every X stage, so waves
//    0-3 wait for them at barriers 3 and 5)
//  * Every (row, unit, gate) accumulator is one lane's fma chain over its list in list order:
//    the result does not depend on the rows per group, the group, ROT or the run.
// Two X stages (XA: x1, x2, y1; XB: h1, h2, y2) and six barriers per step order every reuse
// (the sparse-wide rows).
#include "wrnn_kernels.h"
#include "persist_wide_common.h"
#include "philox.h"
#include "sparse_wide_pack.h"

namespace wrnn {

using wide::WX_D;
using wide::WX_GROUP;

// ---- LDS (floats) -------------------------------------------------------------------------
constexpr int SL_RI = 0;                          // RowInfo of the group's rows (6 words each)
constexpr int SL_VM = SL_RI + 6 * kPWideRows;      // (physical row, step offset) of each row slot
constexpr int SL_FAIL = SL_VM + 2 * kPWideRows;
constexpr int SL_REG = SL_FAIL + 4;               // group, slot, registration result (ints)
constexpr int SL_BIAS = SL_REG + 4;               // b_hh1 [3][16], b_hh2 [3][16], b_fc3 [16 (+16)] of the slot
constexpr int SL_P1R = 512;                       // P1 ring: float4 [16 n][16 j] (one slot, p1_make)
constexpr int SL_GR = SL_P1R + 16 * 16 * 4;       // noise ring: [16 n][16 (C10: 32)] (one slot, noise_make)
constexpr int SL_G = 2048;                        // W_hh1 h1 (r, z, n), W_hh2 h2 (r, z, n): [6][16 n][16 o]
constexpr int SL_XS = kPH + 4;                    // X stage row stride
constexpr int SL_XA = SL_G + 6 * 256;             // X stage A [16 n][SL_XS]: x1, x2, y1
constexpr int SL_XB = SL_XA + kPWideRows * SL_XS; // X stage B: h1, h2, y2
constexpr int SL_STEP_END = SL_XB + kPWideRows * SL_XS;
constexpr int SL_TAB = wsp::kStepBytes / 4;       // the slot's image (sparse_wide_pack.h slot_image)
constexpr int SL_COL = SL_TAB + wsp::kTabBytes / 4;
constexpr int SL_BLK = SL_COL + wsp::kColBytes / 4;
constexpr int SL_TOTAL = SL_BLK + wsp::kListBytes / 4;
static_assert(SL_BIAS + 128 <= SL_P1R && SL_GR + 16 * 32 <= SL_G, "small LDS arrays overflow their region");
static_assert(SL_STEP_END <= SL_TAB, "the per-step arrays exceed the carve's step region (sparse_wide_pack.h kStepBytes)");
static_assert(SL_XA % 4 == 0 && SL_XB % 4 == 0 && SL_XS % 4 == 0 && SL_BLK % 4 == 0, "float4 arrays are 16-byte aligned");
static_assert(SL_TOTAL * 4 <= 160 * 1024, "LDS carve exceeds the CU's 160 KiB (no static LDS)");
static_assert(SL_TOTAL - SL_TAB == wsp::kImgWords, "the image is copied into LDS as it is");
static_assert(wsp::kRows == 16 && wsp::kSlots == kPM && kPWideRows == 16, "a slot's 16 x 16 cells");
static_assert(sizeof(RowInfo) == 24, "RowInfo is 6 words");

// DBG, ROT, C10: as k_persist_wide's (the logit-capture instance; a time-sliced launch; up to 1024
// classes: slot w also owns classes 512 + 16 w .., the lists of set S_FC3B)
template <bool ROT, bool C10, bool DBG>
__global__ __launch_bounds__(kPT, 1) void k_persist_wide_sp(PersistArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    int* sreg = reinterpret_cast<int*>(lds + SL_REG);
    const int tid = threadIdx.x;
    if (tid == 0) {
        int gg, ss;
        sreg[2] = p_register(a.ctl, gg, ss);
        sreg[0] = gg;
        sreg[1] = ss;
    }
    __syncthreads();
    if (!sreg[2]) return;
    const int g = __builtin_amdgcn_readfirstlane(sreg[0]);
    const int w = __builtin_amdgcn_readfirstlane(sreg[1]);
    const int v = __builtin_amdgcn_readfirstlane(tid >> 6);  // wave: polls K-eighth [64v, 64v + 64)
    const int l = tid & 63;
    const int R = a.nr;                  // rows of this group (<= 16)
    const int g0 = a.rb + g;             // group row r = fold row g0 + 8 r
    const int bn = l & 15;               // packet lane: row bn, k-slot l >> 4
    const bool bvalid = bn < R;
    // epilogue cell of threads 0..16R-1: row cn, unit / class 16 w + cul
    const int cn = tid >> 4, cul = tid & 15;
    const bool cell = tid < 16 * R;
    const int cu = 16 * w + cul;
    // product cell of either half of the workgroup: waves 4-7 mirror the cells of waves 0-3
    const int pn = (tid & 255) >> 4;
    const bool pcell = (tid & 255) < 16 * R;
    const int crow = ROT ? a.vmap[g0 + kPG * (cell ? cn : 0)].x : g0 + kPG * (cell ? cn : 0);
    auto wh = [&](unsigned site) {
        unsigned ww = (unsigned)w;
        asm volatile("" : "+s"(ww));
        return site << 28 | ww << 22;
    };
    const rsrc_t xr = mk_rsrc(a.xbuf + (size_t)g * WX_GROUP);
    const bool trace = a.phases != nullptr;
    uint32_t* ph = trace ? a.phases + (size_t)(g * kPM + w) * kPPhases : nullptr;
#define WSTAMP(i)                                                             \
    if (trace && t == a.phase_t && (tid & 255) == 0) {                        \
        ph[(tid >> 8) * 12 + (i)] = p_now();                                  \
        if (tid == 0 && ((i) == 0 || (i) == 10))                              \
            ph[24 + ((i) == 10)] = (uint32_t)__builtin_amdgcn_s_memtime();    \
    }
    // extra stamps of wave 0 at [26, 30): the end of each critical product's gather
#define WXSTAMP(i) \
    if (trace && t == a.phase_t && tid == 0) ph[(i)] = p_now();

    // ---- the slot's lists into LDS ------------------------------------------------------
    {
        const uint4* src = reinterpret_cast<const uint4*>(a.wwide_lds) + (size_t)w * (wsp::kImgWords / 4);
        uint4* dst = reinterpret_cast<uint4*>(lds + SL_TAB);
        for (int i = tid; i < wsp::kImgWords / 4; i += kPT) dst[i] = src[i];
    }
    // ---- state and per-cell constants --------------------------------------------------
    float h1r = 0.f, h2r = 0.f, x1c = 0.f;
    float g1r = 0.f, g1z = 0.f, g1n = 0.f, g2r = 0.f, g2z = 0.f, g2n = 0.f;
    if (cell) {
        h1r = a.st_h1[(size_t)crow * kPH + cu];
        h2r = a.st_h2[(size_t)crow * kPH + cu];
        x1c = a.st_x1[(size_t)crow * kPH + cu];
        g2r = a.st_gh2[(size_t)crow * 3 * kPH + cu];
        g2z = a.st_gh2[(size_t)crow * 3 * kPH + kPH + cu];
        g2n = a.st_gh2[(size_t)crow * 3 * kPH + 2 * kPH + cu];
    }
    if (tid < R) {
        reinterpret_cast<RowInfo*>(lds + SL_RI)[tid] = a.rows[g0 + kPG * tid];
        reinterpret_cast<int2*>(lds + SL_VM)[tid] = ROT ? a.vmap[g0 + kPG * tid] : make_int2(g0 + kPG * tid, 0);
    }
    if (tid == 0) lds[SL_FAIL] = 0.f;
    if (tid < (C10 ? 128 : 112)) {
        const int k = tid < 96 ? tid % 48 : tid - 96;
        const float* src = tid < 48 ? a.b_hh1 : tid < 96 ? a.b_hh2 : a.b_fc3;
        const int cls = 16 * w + (k & 15) + (k >= 16 ? kPH : 0);  // (fc3: tile a, then tile b)
        const int idx = tid < 96 ? (k / 16) * kPH + 16 * w + (k & 15) : cls;
        lds[SL_BIAS + tid] = tid >= 96 && cls >= a.n_classes ? 0.f : src[idx];
    }
    const unsigned o_cons = wide::cons_off(v, l);
    const unsigned o_prod = wide::prod_off(w, cn, cul);
    // publish the cell's value of step s: slot s & 1, and the sentinel into slot (s + 1) & 1
    // (k_persist_wide's pub_if / pub: every lane issues the stores, a lane that does not publish
    // to an out-of-range offset)
    auto pub_if = [&](bool on, int hb, float val, unsigned s) {
        const float u1 = pdpp<0x39>(val), u2 = pdpp<0x4E>(val), u3 = pdpp<0x93>(val);
        const unsigned vo = on && cell && (cul & 3) == 0 ? o_prod : wide::kNoOffset;
        __builtin_amdgcn_raw_buffer_store_b128(
            (u4v){__float_as_uint(val), __float_as_uint(u1), __float_as_uint(u2), __float_as_uint(u3)}, xr, vo,
            wide::slot_base(hb, s), 0);
        __builtin_amdgcn_raw_buffer_store_b128((u4v){kSent, kSent, kSent, kSent}, xr, vo,
                                               wide::slot_base(hb, s + 1u), 0);
    };
    // this lane's 4 packets of a hop (row bn, units 64 v + 16 (l / 16) + 4 p + q) into an X stage
    auto xstore = [&](int X, const u4v (&cc)[4]) {
        float* d = lds + X + bn * SL_XS + 64 * v + 16 * (l >> 4);
#pragma unroll
        for (int p = 0; p < 4; ++p) *reinterpret_cast<u4v*>(d + 4 * p) = cc[p];
    };
    // The sums of K consecutive product sets (from set0) of this thread's cell (row pn, output row
    // cul of the slot) against stage X: each accumulator is one fma chain over its list in list
    // order (ascending column), two blocks of every list in flight per round; a lane whose list
    // has ended keeps its sum (no product with a padding block enters it).
    auto dots = [&](auto kc, int set0, int X, float* out) {
        constexpr int K = decltype(kc)::value;
        const uint32_t* tab = reinterpret_cast<const uint32_t*>(lds + SL_TAB);
        const unsigned short* col = reinterpret_cast<const unsigned short*>(lds + SL_COL);
        const float4* blk = reinterpret_cast<const float4*>(lds + SL_BLK);
        const float* xrow = lds + X + pn * SL_XS;
        int st[K], n[K], nmax = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t e = tab[(set0 + k) * 16 + cul];
            st[k] = (int)(e & 0xffffu);
            n[k] = (int)(e >> 16);
            nmax = n[k] > nmax ? n[k] : nmax;
            out[k] = 0.f;
        }
        for (int i = 0; i < nmax; i += 2) {
#pragma unroll
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const bool on = i + u < n[k];
                    // (a lane past its list reads block 0 of the image: in bounds, never summed;
                    // the column word is masked to the stage's 128 blocks)
                    const int b = on ? st[k] + i + u : 0;
                    const float4 wv = blk[b];
                    const int c = (int)col[b] & (wsp::kColBlocks - 1);
                    const float4 xv = *reinterpret_cast<const float4*>(xrow + 4 * c);
                    float s = out[k];
                    s = fmaf(wv.x, xv.x, s);
                    s = fmaf(wv.y, xv.y, s);
                    s = fmaf(wv.z, xv.z, s);
                    s = fmaf(wv.w, xv.w, s);
                    out[k] = on ? s : out[k];
                }
        }
    };
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    const rsrc_t fcr = mk_rsrc(a.fcond);
    constexpr int NC = C10 ? 32 : 16;  // noise classes per row and slot in the LDS ring
    // per-step operands of the cell (k_persist_wide's prefetch / prefetch_d)
    float pc[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, pg = 0.f, pg2 = 0.f;
    float4 pp = make_float4(0.f, 0.f, 0.f, 0.f), pv = make_float4(0.f, 0.f, 0.f, 0.f);
    auto prefetch = [&](int t) {
        if (!cell) return;
        const RowInfo& ri = reinterpret_cast<const RowInfo*>(lds + SL_RI)[cn];
        const unsigned fo = (unsigned)(p_frame(ri, t, a.hop) * a.cond_width) * 4u;
        int uu = cu;
        asm volatile("" : "+v"(uu));
        pc[0] = bld(fcr, fo + (unsigned)(a.oG2 + uu) * 4u, 0);
        pc[1] = bld(fcr, fo + (unsigned)(a.oG2 + kPH + uu) * 4u, 0);
        pc[2] = bld(fcr, fo + (unsigned)(a.oG2 + 2 * kPH + uu) * 4u, 0);
        pc[3] = bld(fcr, fo + (unsigned)(a.oF1 + uu) * 4u, 0);
        pc[4] = bld(fcr, fo + (unsigned)(a.oF2 + uu) * 4u, 0);
    };
    const rsrc_t vr = mk_rsrc(a.v), w0r = mk_rsrc(a.w0);
    auto prefetch_d = [&]() {
        if (!cell) return;
        int uu = cu;
        asm volatile("" : "+v"(uu));
        pg = lds[SL_GR + cn * NC + cul];
        if constexpr (C10) pg2 = lds[SL_GR + cn * NC + 16 + cul];
        pp = reinterpret_cast<const float4*>(lds + SL_P1R)[cn * 16 + cul];
        pv.x = bld(vr, (unsigned)uu * 4u, 0);
        pv.y = bld(vr, (unsigned)uu * 4u, kPH * 4);
        pv.z = bld(vr, (unsigned)uu * 4u, 2 * kPH * 4);
        pv.w = bld(w0r, (unsigned)uu * 4u, 0);
    };
    // the one-slot LDS rings of waves 4-7 (k_persist_wide's noise_make / p1_make)
    auto noise_make = [&](int n, int j, int tau) {
        const int off = ROT ? reinterpret_cast<const int2*>(lds + SL_VM)[n].y : 0;
        int uu = 16 * w + j;
        asm volatile("" : "+v"(uu));
        const RowInfo& ri = reinterpret_cast<const RowInfo*>(lds + SL_RI)[n];
        const U4 o = philox4x32_10((uint32_t)(uu >> 2), (uint32_t)(tau + off), (uint32_t)ri.fold, ri.stream,
                                   a.k0, a.k1);
        const uint32_t wd = (uu & 3) == 0 ? o.x : (uu & 3) == 1 ? o.y : (uu & 3) == 2 ? o.z : o.w;
        lds[SL_GR + n * NC + j] = __uint_as_float(gumbel_q_of(wd));
        if constexpr (C10) {  // and of class 512 + u
            __builtin_amdgcn_sched_barrier(0);
            const U4 o2 = philox4x32_10((uint32_t)((uu + kPH) >> 2), (uint32_t)(tau + off), (uint32_t)ri.fold,
                                        ri.stream, a.k0, a.k1);
            const uint32_t wd2 = (uu & 3) == 0 ? o2.x : (uu & 3) == 1 ? o2.y : (uu & 3) == 2 ? o2.z : o2.w;
            lds[SL_GR + n * NC + 16 + j] = __uint_as_float(gumbel_q_of(wd2));
        }
    };
    auto p1_make = [&](int n, int j, int tau) {
        const int off = ROT ? reinterpret_cast<const int2*>(lds + SL_VM)[n].y : 0;
        const int tc = tau < a.S - off ? tau : a.S - off - 1;
        int uu = 16 * w + j;
        asm volatile("" : "+v"(uu));
        const RowInfo& ri = reinterpret_cast<const RowInfo*>(lds + SL_RI)[n];
        float4 v;
        if (a.p1q == nullptr) {
            v = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                               mk_rsrc(a.P1 + (size_t)tc * a.B * 4 * kPH),
                                               ((unsigned)(g0 + kPG * n) * 4u * kPH + (unsigned)uu * 4u) * 4u, 0, 0));
        } else {
            const unsigned p = (unsigned)(ri.rel0 + tc);
            const bool in = p < (unsigned)ri.L;  // else the zero tail pad: bias only (zero frame)
            const unsigned f = p / (unsigned)a.hop, sph = in ? p - f * (unsigned)a.hop : 0u;
            const unsigned s0 = in ? (unsigned)ri.fbase - 1u + f + (sph >= (unsigned)a.p1split ? 1u : 0u)
                                   : (unsigned)ri.fbase;
            constexpr unsigned kRow = 4u * kPH * 4u;  // bytes per frame slot
            const unsigned col = (unsigned)uu * 16u;
            const float4 tk = __builtin_bit_cast(
                float4, __builtin_amdgcn_raw_buffer_load_b128(mk_rsrc(a.p1taps), sph * 16u, 0, 0));
            const rsrc_t qr = mk_rsrc(a.p1q);
            float4 tq[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                tq[k] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                       qr, (in ? s0 + (unsigned)k : s0) * kRow + col, 0, 0));
            const float4 ta = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(
                                                             mk_rsrc(a.p1a), (in ? (unsigned)ri.fbase + 1u + f : s0) * kRow + col, 0, 0));
            float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
            const float kk[4] = {tk.x, tk.y, tk.z, tk.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                m.x = fmaf(kk[k], tq[k].x, m.x);
                m.y = fmaf(kk[k], tq[k].y, m.y);
                m.z = fmaf(kk[k], tq[k].z, m.z);
                m.w = fmaf(kk[k], tq[k].w, m.w);
            }
            v = make_float4(p_add(m.x, ta.x), p_add(m.y, ta.y), p_add(m.z, ta.z), p_add(m.w, ta.w));
        }
        reinterpret_cast<float4*>(lds + SL_P1R)[n * 16 + j] = v;
    };
    const bool lo = v < 4;  // waves 0-3 hold the epilogue cells
    __syncthreads();  // RowInfo and the lists in LDS
    // ring prologue: the noise of step t0 and P1(t0 + 1)
    if (!lo && tid - 256 < 16 * R) {
        const int i = tid - 256;
        noise_make(i >> 4, i & 15, a.t0);
        p1_make(i >> 4, i & 15, a.t0 + 1);
    }
    __syncthreads();
    // initial hop E: x1, h1 of step t0 as step t0 + 1 (canonicalised: a signalling NaN in a
    // carried state must not read as the sentinel)
    pub_if(true, WB_X1, __builtin_canonicalizef(x1c), (unsigned)a.t0 + 1u);
    pub_if(true, WB_H1, __builtin_canonicalizef(h1r), (unsigned)a.t0 + 1u);
    if (a.stamps && g == 0 && w == 0 && tid == 0) a.stamps[0] = p_now();
    // a poll of this lane gave up (timeout, PC_ERR raised elsewhere, abort): written to SL_FAIL
    // before the next stage-A barrier only, read by every wave right after it -- the flag's writes
    // and reads never share a barrier interval. The wave finishes the step on whatever its
    // registers hold; every later poll of the step ends within 64 spins of PC_ERR.
    bool fail = false;
    for (int t = a.t0; t < a.t1; ++t) {
        const unsigned seq = (unsigned)t + 1u;
        const unsigned so_x1 = wide::slot_base(WB_X1, seq), so_h1 = wide::slot_base(WB_H1, seq);
        const unsigned so_x2 = wide::slot_base(WB_X2, seq), so_h2 = wide::slot_base(WB_H2, seq);
        const unsigned so_y1 = wide::slot_base(WB_Y1, seq), so_y2 = wide::slot_base(WB_Y2, seq);
        u4v cc[4];
        float x2s = 0.f;  // the value a lo wave publishes (x2, y1, y2)
        WSTAMP(0);
        // ================= hop E: x1 -> XA ===================================================
        fail |= !w_poll(xr, o_cons, so_x1, bvalid, cc, a.ctl, wh(1), (unsigned)t);
        prefetch(t);
        WSTAMP(1);
        xstore(SL_XA, cc);  // (XA: last read by the fc2 products, before barrier 6 of step t - 1)
        if (fail) lds[SL_FAIL] = 1.f;
        lds_barrier();  // 1
        WSTAMP(2);
        if (lds[SL_FAIL] != 0.f) return;
        // h1 (published with x1, read above) loads now: in flight over the GRU2 products
        w_issue(xr, o_cons, so_h1, bvalid, cc);
        // ================= W_ih2[:, :512] x1, GRU2 epilogue (waves 0-3) -> publish x2, h2 =====
        if (lo) {
            float x2 = 0.f;
            if (cell) {
                float gi[3];
                dots(I3(), wsp::S_IH2, SL_XA, gi);
                WXSTAMP(26);
#pragma unroll
                for (int j = 0; j < 3; ++j) gi[j] = p_add(gi[j], pc[j]);
                h2r = p_gru(gi[0], gi[1], gi[2], g2r, g2z, g2n, h2r);
                x2 = p_add(x1c, h2r);
            }
            x2s = x2;
        }
        pub_if(lo, WB_X2, x2s, seq);
        pub_if(lo, WB_H2, h2r, seq);
        WSTAMP(3);
        // h1 -> XB (XB: last read by the fc3 products of step t - 1, before this step's barrier 1)
        fail |= !w_poll(xr, o_cons, so_h1, bvalid, cc, a.ctl, wh(2), (unsigned)t, true);
        xstore(SL_XB, cc);
        lds_barrier();  // 2
        // ================= W_hh1 h1 -> gh1 (waves 4-7) ========================================
        if (!lo && pcell) {
            float gh[3];
            dots(I3(), wsp::S_HH1, SL_XB, gh);
            // (G 0-2: last read by waves 0-3 in hop D of step t - 1, before this step's barrier 1)
#pragma unroll
            for (int j = 0; j < 3; ++j) lds[SL_G + (j * 16 + pn) * 16 + cul] = gh[j];
        }
        // ================= hop A: x2 -> XA (its GRU2 reads ended before barrier 2) ============
        fail |= !w_poll(xr, o_cons, so_x2, bvalid, cc, a.ctl, wh(3), (unsigned)t);
        WSTAMP(4);
        xstore(SL_XA, cc);
        lds_barrier();  // 3
        WSTAMP(5);
        // h2 (published with x2) loads now: in flight over fc1
        w_issue(xr, o_cons, so_h2, bvalid, cc);
        // fc1 x2, epilogue (waves 0-3): y1 = relu(fc1 x2 + fc1[:, 512:] a3 + b) -> publish
        if (lo) {
            float y = 0.f;
            if (cell) {
                float s;
                dots(I1(), wsp::S_FC1, SL_XA, &s);
                WXSTAMP(27);
                y = p_add(s, pc[3]);
                y = y > 0.f ? y : 0.f;
            }
            x2s = y;
        }
        pub_if(lo, WB_Y1, x2s, seq);
        // h2 -> XB (its W_hh1 reads by waves 4-7 ended before barrier 3)
        fail |= !w_poll(xr, o_cons, so_h2, bvalid, cc, a.ctl, wh(5), (unsigned)t, true);
        xstore(SL_XB, cc);
        lds_barrier();  // 4
        // ================= W_hh2 h2 -> gh2 (waves 4-7) ========================================
        if (!lo && pcell) {
            float gh[3];
            dots(I3(), wsp::S_HH2, SL_XB, gh);
#pragma unroll
            for (int j = 0; j < 3; ++j) lds[SL_G + ((3 + j) * 16 + pn) * 16 + cul] = gh[j];
        }
        // ================= hop B: y1 -> XA (its fc1 reads ended before barrier 4) =============
        fail |= !w_poll(xr, o_cons, so_y1, bvalid, cc, a.ctl, wh(6), (unsigned)t);
        WSTAMP(6);
        xstore(SL_XA, cc);
        lds_barrier();  // 5
        WSTAMP(7);
        // fc2 y1, epilogue (waves 0-3): y2 = relu(fc2 y1 + fc2[:, 512:] a4 + b) -> publish
        if (lo) {
            float y = 0.f;
            if (cell) {
                float s;
                dots(I1(), wsp::S_FC2, SL_XA, &s);
                WXSTAMP(28);
                y = p_add(s, pc[4]);
                y = y > 0.f ? y : 0.f;
            }
            x2s = y;
        }
        pub_if(lo, WB_Y2, x2s, seq);
        // ================= hop C: y2 -> XB (its W_hh2 reads ended before barrier 5) ===========
        fail |= !w_poll(xr, o_cons, so_y2, bvalid, cc, a.ctl, wh(8), (unsigned)t);
        WSTAMP(8);
        xstore(SL_XB, cc);
        // the rings' values of this step (waves 4-7 rewrite them after barrier 6)
        prefetch_d();
        lds_barrier();  // 6
        WSTAMP(9);
        if (lo) {
            // fc3 y2 and its epilogue: the candidate key of the slot's 16 (C10: 32) classes per row,
            // max over the row's DPP row of 16 lanes, published with the step tag by lane cul == 0
            uint32_t kh = 0, kl = 0;
            if (cell && cu < a.n_classes) {
                float s[C10 ? 2 : 1];
                if constexpr (C10) dots(I2(), wsp::S_FC3, SL_XB, s);
                else dots(I1(), wsp::S_FC3, SL_XB, s);
                WXSTAMP(29);
                const float lg = p_add(s[0], lds[SL_BIAS + 96 + cul]);
                p_dbg_logit<DBG>(a.dbg, t + (ROT ? reinterpret_cast<const int2*>(lds + SL_VM)[cn].y : 0), crow, cu,
                                 a.B, a.n_classes, lg);
                const CandKey k = cand_key(lg, __float_as_uint(pg), cu);
                kh = k.hi;
                kl = k.lo;
                if constexpr (C10) {  // class 512 + cu
                    if (kPH + cu < a.n_classes) {
                        const float lg2 = p_add(s[1], lds[SL_BIAS + 112 + cul]);
                        p_dbg_logit<DBG>(a.dbg, t + (ROT ? reinterpret_cast<const int2*>(lds + SL_VM)[cn].y : 0),
                                         crow, kPH + cu, a.B, a.n_classes, lg2);
                        int c2 = kPH + cu;
                        asm volatile("" : "+v"(c2));
                        const CandKey k2 = cand_key(lg2, __float_as_uint(pg2), c2);
                        kmax_take(kh, kl, k2.hi, k2.lo);
                    }
                }
            }
            row16_kmax(kh, kl);
            if (cell && cul == 0)
                __builtin_amdgcn_raw_buffer_store_b64((u2v){kh, kl | key_tag(seq)}, xr, wide::cand_off(cn, w),
                                                      WX_D * 4, 0);
            // gh1 = W_hh1 h1 + b_hh1 (for GRU1 below) and gh2 = W_hh2 h2 + b_hh2 (the next GRU2):
            // waves 4-7 wrote G before barriers 3 and 5, and rewrite it after the next step's
            // barriers 2 and 4
            if (cell) {
                float gs[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) gs[j] = p_add(lds[SL_G + (j * 16 + cn) * 16 + cul], lds[SL_BIAS + 16 * j + cul]);
                g1r = gs[0];
                g1z = gs[1];
                g1n = gs[2];
                g2r = gs[3];
                g2z = gs[4];
                g2n = gs[5];
            }
            // ============= hop D: sample of step t, per cell wave for its own 4 rows ========
            u4v q;
            fail |= !poll_cand_couple(xr, cell, wide::cand_off(cn, 2 * cul), WX_D * 4, key_tag(seq), a.ctl, wh(9),
                                      (unsigned)t, false, q);
            uint32_t bh = q.x, bl = q.y;
            kmax_take(bh, bl, q.z, q.w);
            row16_kmax(bh, bl);
            const int bi = key_cls(bl);
            const float x = bits_sample_of(bi, a.n_classes);
            if (w == 0 && cell && cul == 0) {
                int nn = cn;
                asm volatile("" : "+v"(nn));
                const int2 vm = reinterpret_cast<const int2*>(lds + SL_VM)[nn];
                const unsigned ro = (unsigned)(vm.x * a.ld + vm.y);
                __builtin_amdgcn_raw_buffer_store_b16((unsigned short)bi, mk_rsrc(a.labels), ro * 2u,
                                                      (unsigned)t * 2u, 0);
                bst(x, mk_rsrc(a.samples), ro * 4u, (unsigned)t * 4u);
            }
            WSTAMP(10);
            // ============= GRU1 of step t + 1 for the slot's units -> publish x1, h1 ========
            float x1 = 0.f;
            if (cell) {
                h1r = p_gru(fmaf(pv.x, x, pp.x), fmaf(pv.y, x, pp.y), fmaf(pv.z, x, pp.z), g1r, g1z, g1n, h1r);
                x1 = p_add(fmaf(pv.w, x, pp.w), h1r);
                x1c = x1;
            }
            pub_if(true, WB_X1, x1, seq + 1u);
            pub_if(true, WB_H1, h1r, seq + 1u);
        } else {
            // waves 4-7: the noise of step t + 1 and P1(t + 2) into the one-slot LDS rings (waves
            // 0-3 read this step's values in prefetch_d, before barrier 6)
            const int i = tid - 256;
            if (i < 16 * R) {
                noise_make(i >> 4, i & 15, t + 1);
                p1_make(i >> 4, i & 15, t + 2);
            }
        }
        if (w == 0 && tid == 0) {
            if (g == 0) p_progress(a.progress, a.prog_base, t);
            if (p_abort(a.ctl, a.progress, t)) fail = true;  // seen at the next stage-A check
        }
        WSTAMP(11);
    }
#undef WSTAMP
#undef WXSTAMP
    if (a.stamps && g == 0 && w == 0 && tid == 0) a.stamps[1] = p_now();
    // ---- the rows' state for a later launch (k_persist's chunk-state layout) ----------------
    if (fail) lds[SL_FAIL] = 1.f;
    __syncthreads();
    if ((ROT || a.t1 < a.S) && cell && lds[SL_FAIL] == 0.f) {
        int nn = cn;
        asm volatile("" : "+v"(nn));
        const int row = reinterpret_cast<const int2*>(lds + SL_VM)[nn].x;
        a.st_x1[(size_t)row * kPH + cu] = x1c;
        a.st_h1[(size_t)row * kPH + cu] = h1r;
        a.st_h2[(size_t)row * kPH + cu] = h2r;
        a.st_gh2[(size_t)row * 3 * kPH + cu] = g2r;
        a.st_gh2[(size_t)row * 3 * kPH + kPH + cu] = g2z;
        a.st_gh2[(size_t)row * 3 * kPH + 2 * kPH + cu] = g2n;
    }
}

size_t persist_wide_sp_lds_bytes() { return (size_t)SL_TOTAL * sizeof(float); }

// scratch bytes of the production instances (0: spill-free), -1 on a query error
int persist_wide_sp_scratch(bool rot, bool c10) {
    const void* f = rot ? (c10 ? (const void*)k_persist_wide_sp<true, true, false>
                               : (const void*)k_persist_wide_sp<true, false, false>)
                        : (c10 ? (const void*)k_persist_wide_sp<false, true, false>
                               : (const void*)k_persist_wide_sp<false, false, false>);
    return persist_fn_scratch(f);
}

// a.wwide_lds: the slots' images ([kPM][wsp::kImgWords] words, sparse_wide_pack.h slot_image)
hipError_t launch_persist_wide_sp(const PersistArgs& a, hipStream_t s) {
    // (the wide launch's argument check; then RAW only, 512 or 1024 classes, the list images)
    if (!persist_wide_args_ok(a) || a.mode != 0 || (a.n_classes != kPM * 16 && a.n_classes != 2 * kPM * 16) ||
        a.wwide_lds == nullptr)
        return hipErrorInvalidValue;
    const size_t lb = persist_wide_sp_lds_bytes();
    const bool dbg = a.dbg.out != nullptr;
    if (a.n_classes > kPM * 16) {
        if (a.vmap) return dbg ? persist_launch<k_persist_wide_sp<true, true, true>>(lb, a, s)
                               : persist_launch<k_persist_wide_sp<true, true, false>>(lb, a, s);
        return dbg ? persist_launch<k_persist_wide_sp<false, true, true>>(lb, a, s)
                   : persist_launch<k_persist_wide_sp<false, true, false>>(lb, a, s);
    }
    if (a.vmap) return dbg ? persist_launch<k_persist_wide_sp<true, false, true>>(lb, a, s)
                           : persist_launch<k_persist_wide_sp<true, false, false>>(lb, a, s);
    return dbg ? persist_launch<k_persist_wide_sp<false, false, true>>(lb, a, s)
               : persist_launch<k_persist_wide_sp<false, false, false>>(lb, a, s);
}

}  // namespace wrnn
