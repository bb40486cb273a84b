// Step helpers shared by the three wide MFMA recurrence kernels (kernels_persist_wide.hip,
// kernels_persist_wide_rr.hip, kernels_persist_wide_gen.hip): the MFMA operand accessors, the
// sentinel of the untagged vector packets, the bounded-spin timeout report, the two polls of the
// sample hop and the samplers whose arithmetic is part of the parity contract. One definition
// each, so a fix to the MOL arithmetic or to the timeout report is made once.
#pragma once

#include "persist_common.h"
#include "wide_layout.h"

namespace wrnn {

typedef float v4f __attribute__((ext_vector_type(4)));

// a signalling NaN: no arithmetic result is ever this (an unwritten packet slot holds it)
constexpr unsigned kSent = 0x7fbadbadu;
// lanes without a packet: outside every buffer (mk_rsrc num_records), so a load reads 0 and a
// store is dropped (the value lives in wide_layout.h, with the host-side layout checks)
constexpr unsigned kNoOff = wide::kNoOffset;

__device__ __forceinline__ v4f mfma4(float a, float b, v4f c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float f4c(const float4& q, int i) {
    return i == 0 ? q.x : i == 1 ? q.y : i == 2 ? q.z : q.w;
}
// component i of a polled packet as the float it carries
__device__ __forceinline__ float u4c(const u4v& q, int i) {
    return __uint_as_float(i == 0 ? q.x : i == 1 ? q.y : i == 2 ? q.z : q.w);
}
// Partial tiles: element (row n, column o) of a [16][16] tile sits at n * 16 + wsw(n, o), the
// 16-byte column slots XOR-swizzled by row: an MFMA lane's 16-byte store (row bn, columns
// 4c .. 4c + 3) and the epilogue's row reads are then both conflict-free (a ds_write_b128 is
// served 8 contiguous lanes at a time on 32 banks: unswizzled, rows 64 B apart put 8 rows on 2
// slots -- 4-way, 24 extra LDS cycles per store, ~2300 per CU and step; SQ_LDS_BANK_CONFLICT,
// profiles/r03/pmc/c4_sq)
__device__ __forceinline__ int wsw(int n, int o) { return ((((o >> 2) ^ (n >> 1)) & 3) << 2) | (o & 3); }

__device__ __forceinline__ bool packet_ready(const u4v& q) {
    // bitwise: the short-circuit form compiled to a branch and a wait per packet
    return (q.x != kSent) & (q.y != kSent) & (q.z != kSent) & (q.w != kSent);
}

// LDS-only workgroup barrier: no wait on outstanding global loads (prefetches stay in flight)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// A bounded spin has expired (what follows `(++nsp & 63) == 0 && (ld_sc1_u(ctl + PC_ERR) ||
// p_now() - t0 > kSpinTicks)`): the first wave of the call to get here records its site in
// PC_WHERE (`where`: site << 28 | slot << 22; the wave is added here), whether its packets were
// missing (PC_WHERE + 1) and the step (PC_WHERE + 2, all 32 bits) for the error message; every
// wave raises PC_ERR to 2. Called by whole waves.
// (the wave index read back as a scalar: a per-lane form held VGPRs across the step loop)
__device__ __forceinline__ void spin_give_up(unsigned* ctl, unsigned where, unsigned step, bool missing) {
    const unsigned wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0) {
        if (!ld_sc1_u(ctl + PC_ERR) && atomicCAS(ctl + PC_WHERE, 0u, where | (wv << 19)) == 0u) {
            ctl[PC_WHERE + 1] = missing ? 1u : 0u;
            ctl[PC_WHERE + 2] = step;
        }
        atomicMax(ctl + PC_ERR, 2u);
    }
}

// The vectors a step of the fatchord wide kernels publishes (kernels_persist_wide.hip,
// kernels_persist_wide_sp.hip): one slot pair each in the exchange area (wide_layout.h)
enum WBuf : int { WB_X1 = 0, WB_H1, WB_X2, WB_H2, WB_Y1, WB_Y2, WB_N };
static_assert(WB_N == wide::kBufs, "one slot pair per published vector");

// Poll this lane's 4 packets of one hop buffer slot (byte offset of packet 0: voff; packet p at
// voff + 1 KiB p; so: the buffer and slot) until no value is the sentinel, all 4 in flight on
// every pass. Lanes with valid == false (rows beyond the group's count) contribute zeros.
// Why a sentinel is enough (no step tags): a producer writes step s into slot s & 1 and the
// sentinel into slot (s + 1) & 1 (pub). Its next poll waits for every older vector memory
// operation of the wave (vmcnt counts stores on gfx9), so that reset is in L2 before it
// publishes anything later; a consumer polls slot (s + 1) & 1 for step s + 1 only after it has
// read such a later publication, so it sees the reset or the new value, never step s - 1. And
// slot s & 1 is rewritten (step s + 2) only after every consumer has published past its reads
// of step s.
// The 4 packet loads of a poll round. Unconditional: a lane without an operand loads from an
// out-of-range offset, which reads 0 ("ready"), so every path carries the same loads and the
// compiler's waits stay counted (a branch around them made the waits after it conservative).
// w_issue alone: the first round issued early, for an off-path operand published long before
// its use, checked later by w_poll with pre = true.
__device__ __forceinline__ void w_issue(rsrc_t xr, unsigned voff, unsigned so, bool valid, u4v (&cc)[4]) {
    unsigned vo = valid ? voff : wide::kNoOffset;
    asm volatile("" : "+v"(vo));
#pragma unroll
    for (int i = 0; i < 4; ++i) cc[i] = __builtin_amdgcn_raw_buffer_load_b128(xr, vo + 1024u * i, so, kCpNT);
}
// Packet i of a poll round alone (see w_issue): issued into a packet register an off-path
// product has finished reading, so a critical hop's first round needs no extra registers.
__device__ __forceinline__ void w_issue1(rsrc_t xr, unsigned voff, unsigned so, bool valid, u4v& c, int i) {
    unsigned vo = valid ? voff : wide::kNoOffset;
    asm volatile("" : "+v"(vo));
    c = __builtin_amdgcn_raw_buffer_load_b128(xr, vo + 1024u * i, so, kCpNT);
}
// On a timeout the first poller records its site, whether its packets were missing and the step
// (spin_give_up).
__device__ __forceinline__ bool w_poll(rsrc_t xr, unsigned voff, unsigned so, bool valid, u4v (&cc)[4],
                                       unsigned* ctl, unsigned where, unsigned step, bool pre = false) {
    const unsigned t0 = p_now();
    unsigned nsp = 0;
    if (!pre) w_issue(xr, voff, so, valid, cc);
    {
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 4; ++i) ok &= packet_ready(cc[i]);
        if (__all(ok)) return true;
    }
    while (true) {
        // every packet reloaded per spin: a lane's 4 packets come from one producer slot's one
        // store instruction, so when packet 0 lands the others have too and no second L2 round
        // trip follows (round 3 A/B: 11.33 against 11.48 us per step spinning on packet 0,
        // profiles/r03/ab_spin/)
        w_issue(xr, voff, so, valid, cc);
        {
            bool ok = true;
#pragma unroll
            for (int i = 0; i < 4; ++i) ok &= packet_ready(cc[i]);
            if (__all(ok)) return true;
        }
        if ((++nsp & 63) == 0 && (ld_sc1_u(ctl + PC_ERR) || p_now() - t0 > kSpinTicks)) {
            bool mok = true;
#pragma unroll
            for (int i = 0; i < 4; ++i) mok &= packet_ready(cc[i]);
            spin_give_up(ctl, where, step, !__all(mok));
            return false;
        }
    }
}

// Sample hop of the MOL / Beta heads: lane (row, cul) polls the tagged pairs (float bits, the
// whole step tag seq) of logits cul (at byte offset va, wanted where ra) and 16 + cul (vb, rb) of
// its row in the area at scalar offset so; a lane without a logit passes kNoOff (reads 0, not
// waited for). Bounded; false after a give-up.
__device__ __forceinline__ bool poll_logit_pairs(rsrc_t xr, unsigned va, unsigned vb, unsigned so, bool ra, bool rb,
                                                 unsigned seq, unsigned* ctl, unsigned where, unsigned step,
                                                 bool missing, u2v& qa, u2v& qb) {
    asm volatile("" : "+v"(va), "+v"(vb));
    const unsigned t0 = p_now();
    unsigned nsp = 0;
    while (true) {
        qa = __builtin_amdgcn_raw_buffer_load_b64(xr, va, so, kCpNT);
        qb = __builtin_amdgcn_raw_buffer_load_b64(xr, vb, so, kCpNT);
        if (__all((!ra | (qa.y == seq)) & (!rb | (qb.y == seq)))) return true;
        if ((++nsp & 63) == 0 && (ld_sc1_u(ctl + PC_ERR) || p_now() - t0 > kSpinTicks)) {
            spin_give_up(ctl, where, step, missing);
            return false;
        }
    }
}

// Sample hop of the categorical heads: a polling lane (on) reads the candidate couple (two keys
// of cand_key.h, 16 bytes at byte offset off) until both carry the step's key tag `want`; the
// other lanes keep {0, want, 0, want}. Bounded; false after a give-up.
__device__ __forceinline__ bool poll_cand_couple(rsrc_t xr, bool on, unsigned off, unsigned so, unsigned want,
                                                 unsigned* ctl, unsigned where, unsigned step, bool missing,
                                                 u4v& q) {
    q = (u4v){0u, want, 0u, want};
    const unsigned t0 = p_now();
    unsigned nsp = 0;
    while (true) {
        if (on) {
            unsigned vo = off;
            asm volatile("" : "+v"(vo));
            q = __builtin_amdgcn_raw_buffer_load_b128(xr, vo, so, kCpNT);
        }
        if (__all(((q.y & kKeyTagMask) == want) & ((q.w & kKeyTagMask) == want))) return true;
        if ((++nsp & 63) == 0 && (ld_sc1_u(ctl + PC_ERR) || p_now() - t0 > kSpinTicks)) {
            spin_give_up(ctl, where, step, missing);
            return false;
        }
    }
}

// The mixture-of-logistics sample of a row held by its 16 lanes (lane cul: logits la = l[cul],
// lb = l[16 + cul]; pg: draw cul of the row's 11): k_persist's operations in its order
// (kernels_persist.hip, "MOL:"; vocoder/distribution.py:104-140) -- first max over the 10 mixture
// logits minus their draws, mean, log-scale clamp, mean + exp(ls) lu, clamp to [-1, 1]. Every
// lane of the row returns the sample.
__device__ __forceinline__ float mol_sample_row16(float la, float lb, float pg, int cul, int lane) {
    float bv;
    {
#pragma clang fp contract(off)
        bv = cul < 10 ? la - pg : -INFINITY;
    }
    int bi = cul < 10 ? cul : 0x7fffffff;
    row16_argmax(bv, bi);  // first max over k < 10; every lane of the row gets it
    bi = bi < 10 ? bi : 0;
    const int base = lane & 48;  // lane 0 of this lane's row
    // l[10 + bi]: the first value of lane 10 + bi, or the second of lane bi - 6
    const float m0 = __shfl(la, base + ((10 + bi) & 15)), m1 = __shfl(lb, base + ((10 + bi) & 15));
    const float mean = bi < 6 ? m0 : m1;
    float ls = __shfl(lb, base + 4 + bi);  // l[20 + bi]: the second value of lane 4 + bi
    const float lu = __shfl(pg, base + 10);
    float x;
    {
#pragma clang fp contract(off)
        const float lsmin = -32.23619130191664f;  // float(np.log(1e-14))
        ls = ls < lsmin ? lsmin : ls;
        x = mean + expf(ls) * lu;
        x = x < -1.f ? -1.f : x;
        x = x > 1.f ? 1.f : x;
    }
    return x;
}

// the categorical sample of class bi of n: 2 bi / (n - 1) - 1, un-contracted
__device__ __forceinline__ float bits_sample_of(int bi, int n_classes) {
#pragma clang fp contract(off)
    return (2.0f * (float)bi) / (float)(n_classes - 1) - 1.0f;
}

}  // namespace wrnn
