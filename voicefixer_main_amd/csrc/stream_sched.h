// stream_sched.h -- the bookkeeping of a streaming session (vfx_stream_*): which chunk of which slot is due, how the rows of a group
// are ordered, what every launch table of stream.hip contains, back-pressure and the refusals.  No HIP call and no device memory in
// here: the scheduler works on sample counts alone, so it is compiled and driven on the host by tests/stream_sched_main.cpp.
//
// Coordinates are sample indices of a slot's stream (int64).  A ring cell of sample n is n % capacity; a stream that is opened
// again starts at n = 0.  The two modes restate voicefixer_main_amd/chunker.py:
//   overlap-add (mode 0, par = hop H): chunk k >= 1 is x[kH - W, kH); due at kH fed samples, at close up to k = (L + W - 1) / H;
//                                      sample n is final once chunk (n + W) / H is stitched.
//   boxcar      (mode 1, par = margin M): frame 0 is x[0, W + M) -> [0, W); frame k is x[kW - M, (k+1)W + M) -> [kW, (k+1)W);
//                                      at close the last of ceil(L / W) frames runs at M + last (or M + W) samples, no back margin.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace vfx {

enum { STREAM_OLA = 0, STREAM_BOXCAR = 1 };

// packed block buffer <-> ring: `count` samples at `off` of the packed buffer, ring cell `pos` onwards (wraps)
struct StreamCopyRow {
  int slot;
  int64_t off, count, pos;
};
// one row of a chunk batch: samples [start, start + row length) of the slot, zeros outside [0, valid_end); pos = cell of `start`
struct StreamGatherRow {
  int slot;
  int64_t start, valid_end, pos;
};
// overlap-add stitch, one per slot of the group: rows [row0, row0 + nk) are its chunks k0, k0 + 1, ...  Every n of [span0, span1)
// is summed; cells below prior_end hold a partial sum, n < final_end is final (written to the output ring when n < out_limit), the
// rest is stored as a partial sum.  `parity` is the half of the accumulator that is read; the other half is written.
struct StreamOlaRow {
  int slot, row0, nk, parity;
  int64_t k0, span0, span1, prior_end, final_end, out_limit;
};
// boxcar stitch, one per row: samples [off, off + count) of row `row` are output samples n0 onwards
struct StreamBoxRow {
  int slot, row, off;
  int64_t count, n0;
};

class StreamSched {
 public:
  StreamSched(int slots, int mode, int win, int par, int64_t cap_in, int64_t cap_out);
  static bool check_geometry(int slots, int mode, int win, int par, int64_t cap_in, int64_t cap_out, std::string* err);

  // every call returns false with `error` set and nothing changed when it is refused
  bool open(int* slot);
  bool push(int n, const int* slots, const int64_t* counts, std::vector<StreamCopyRow>* rows);
  bool close(int slot);
  bool next(int max_rows, std::vector<StreamGatherRow>* rows, int* row_len);   // 0 rows: nothing is due
  bool put(std::vector<StreamOlaRow>* ola, std::vector<StreamBoxRow>* box);
  bool available(int slot, int64_t* n) const;
  bool room(int slot, int64_t* n) const;   // what a push to the slot may hold now
  bool pop(int n, const int* slots, const int64_t* max_counts, std::vector<StreamCopyRow>* rows, int64_t* counts_out);
  bool state(int slot, int64_t* fed, int64_t* released) const;

  std::string error;

 private:
  enum { FREE = 0, OPEN = 1, CLOSING = 2, CLOSED = 3 };   // CLOSED: flushed; open() takes it again once it is popped empty
  struct Slot {
    int state = FREE;
    int parity = 0;
    int64_t fed = 0, consumed = 0, next = 0, released = 0, popped = 0;
  };
  struct Chunk {   // what the scheduler knows of one due chunk
    int64_t start, valid_end, consumed_after, release_end;
    int len, off;
    int64_t count, n0;   // boxcar: the kept part of the row and where it goes; overlap-add: n0 = end of the final span
  };
  struct Item {
    int slot;
    int64_t k;
    Chunk c;
  };
  bool due(const Slot& s, int64_t k, Chunk* c) const;
  bool fail(const char* fmt, ...);
  bool slot_ok(int slot, const char* what);

  int slots_, mode_, win_, par_;
  int64_t cap_in_, cap_out_;
  std::vector<Slot> s_;
  std::vector<Item> group_;   // the rows handed out by next() and not yet put()
};

}  // namespace vfx
