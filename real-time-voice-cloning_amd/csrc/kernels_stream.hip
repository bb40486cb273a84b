// Small kernels of the streaming sessions (stream.hip) around the streaming
// instances of k_persist (kernels_persist.hip launch_persist_stream): the GRU1 a session's
// launch starts from, and the Gumbel noise of exactly the step windows a launch runs.
#include "wrnn_kernels.h"
#include "persist_common.h"
#include "philox.h"

namespace wrnn {

// GRU1 of a session's step0 > 0 from the operands its last launch saved (persist_body STRM) and
// P1(step0): the arithmetic of the in-kernel GRU1 (p_gru on fmaf(v, x, P1); x1 = (cI + w0 x) + h1).
// Step 0 is k_persist_init's.
__global__ __launch_bounds__(kPT) void k_persist_stream_resume(const StreamGroup* sg, const float* v,
                                                               const float* w0) {
    const StreamGroup s = sg[blockIdx.x];
    if (s.steps <= 0 || s.step0 == 0) return;
    constexpr int H = kPH;
    const int j = threadIdx.x;
    const float* sv = s.st + 6 * H;
    const float* P1 = s.P1 + (size_t)j * 4;
    const float x = sv[4 * H];
    const float hn = p_gru(fmaf(v[j], x, P1[0]), fmaf(v[H + j], x, P1[1]), fmaf(v[2 * H + j], x, P1[2]),
                           sv[H + j], sv[2 * H + j], sv[3 * H + j], sv[j]);
    s.st[H + j] = hn;
    s.st[j] = p_add(fmaf(w0[j], x, P1[3]), hn);
}

hipError_t launch_stream_resume(const StreamGroup* sg, int n, const float* v, const float* w0, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n > kPG) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_persist_stream_resume, dim3(n), dim3(kPT), 0, s, sg, v, w0);
    return hipGetLastError();
}

// k_gumbel for the step windows of a streaming launch: group blockIdx.y, window step t is the
// stream's absolute step step0 + t (fold 0), stored at [t][n] of the session's own window buffer
__global__ __launch_bounds__(256) void k_gumbel_stream(const StreamGroup* sg, int ng) {
    const StreamGroup s = sg[blockIdx.y];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // (t, k4)
    if (i >= (size_t)(s.steps > 0 ? s.steps : 0) * ng) return;
    const int k4 = (int)(i % ng), t = (int)(i / ng);
    const U4 o = philox4x32_10((uint32_t)k4, (uint32_t)(s.step0 + t), 0u, s.stream, s.k0, s.k1);
    reinterpret_cast<uint4*>(s.gumbel)[i] =
        make_uint4(gumbel_q_of(o.x), gumbel_q_of(o.y), gumbel_q_of(o.z), gumbel_q_of(o.w));
}

hipError_t launch_gumbel_stream(const StreamGroup* sg, int n, int max_steps, int n_classes, hipStream_t s) {
    if (n_classes % 4 || n < 0 || n > kPG) return hipErrorInvalidValue;
    const int ng = n_classes / 4;
    const size_t total = (size_t)max_steps * ng;
    if (total == 0 || n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gumbel_stream, dim3((unsigned)((total + 255) / 256), n), dim3(256), 0, s, sg, ng);
    return hipGetLastError();
}

}  // namespace wrnn
