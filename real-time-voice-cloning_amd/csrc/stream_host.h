// Readiness rule of the streaming sessions (stream.hip): host-only C++, shared by
// the runtime and wrnn_debug_stream_ready so the two cannot drift.
#pragma once
#include <stdint.h>

namespace wrnn {

// Frames a step's frame must have behind it before the step may run: the MelResNet row of frame
// f reads mel frames up to f + pad (conv_in; the residual blocks are 1 x 1), and the in-kernel
// P1 taps of a step in frame f read the projections of frames up to f + tap_reach.
inline int stream_lookahead(int pad, int tap_reach) { return pad > tap_reach ? pad : tap_reach; }

// Steps of a session that may run once `frames` frames are pushed: all T * hop after the last
// push, else the steps of the frames that have `lookahead` frames behind them.
inline int64_t stream_ready_steps(int frames, int last, int hop, int lookahead) {
    if (last) return (int64_t)frames * hop;
    const int f = frames - lookahead;
    return f > 0 ? (int64_t)f * hop : 0;
}

}  // namespace wrnn
