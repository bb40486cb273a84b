// Host-only part of the streaming sessions: the readiness rule's ABI entry point (no device).
#include "stream_host.h"

#include "wavernn_mi355x.h"

extern "C" int wrnn_internal_fail(int code, const char* msg);

extern "C" int wrnn_debug_stream_ready(int frames, int last, int hop, int lookahead, int64_t* steps) {
    if (!steps) return wrnn_internal_fail(WRNN_ERR_INVALID, "null steps");
    if (frames < 0 || hop <= 0 || lookahead < 0)
        return wrnn_internal_fail(WRNN_ERR_INVALID, "frames, hop and lookahead must not be negative (hop > 0)");
    *steps = wrnn::stream_ready_steps(frames, last != 0, hop, lookahead);
    return WRNN_OK;
}
