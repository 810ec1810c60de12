// stream.h -- what api.cpp needs of stream.hip: the launches that take the tables of stream_sched.h.
#pragma once
#include "stream_sched.h"
#include "vfx_internal.h"

namespace vfx {

// rows per launch: the table travels in the kernel's arguments (64 x 32 bytes, 32 x 64 bytes)
constexpr int kStreamRows = 64;
constexpr int kStreamOlaRows = 32;

void launch_stream_copy(bool to_ring, float* ring, int cap, float* packed, const std::vector<StreamCopyRow>& rows, hipStream_t s);
void launch_stream_gather(const float* ring, int cap, int row_len, float* chunks, const std::vector<StreamGatherRow>& rows,
                          hipStream_t s);
void launch_stream_ola(const float* frames, const float* window, float scale, int W, int H, float* acc, float* out, int cap_out,
                       const std::vector<StreamOlaRow>& rows, hipStream_t s);
void launch_stream_box(const float* frames, int row_len, const float* window, float scale, float* out, int cap_out,
                       const std::vector<StreamBoxRow>& rows, hipStream_t s);

}  // namespace vfx
