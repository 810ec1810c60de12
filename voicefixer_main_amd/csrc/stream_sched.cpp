// stream_sched.cpp -- see stream_sched.h.  Host arithmetic only.
#include "stream_sched.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>

namespace vfx {

bool StreamSched::check_geometry(int slots, int mode, int win, int par, int64_t cap_in, int64_t cap_out, std::string* err) {
  char buf[256];
  buf[0] = 0;
  if (slots < 1)
    snprintf(buf, sizeof(buf), "a session needs at least one slot, got %d", slots);
  else if (mode != STREAM_OLA && mode != STREAM_BOXCAR)
    snprintf(buf, sizeof(buf), "mode %d is neither overlap-add (0) nor boxcar (1)", mode);
  else if (win < 2 || win % 2 != 0)
    snprintf(buf, sizeof(buf), "Window size must be even, got %d", win);
  else if (mode == STREAM_OLA && (par < 1 || par > win))
    snprintf(buf, sizeof(buf), "hop size %d is outside [1, window size %d]", par, win);
  else if (mode == STREAM_BOXCAR && (par < 0 || par > (1 << 28)))
    snprintf(buf, sizeof(buf), "in_margin %d is negative or too large", par);
  else if (win > (1 << 28))
    snprintf(buf, sizeof(buf), "window size %d is too large", win);
  else {
    const int64_t need = mode == STREAM_OLA ? win : (int64_t)win + 2 * par;
    if (cap_in < need || cap_in > 0x7fffffff)
      snprintf(buf, sizeof(buf), "the input ring holds %lld samples; one chunk needs %lld (and at most 2^31 - 1 fit)", (long long)cap_in,
               (long long)need);
    else if (cap_out < win || cap_out > 0x7fffffff)
      snprintf(buf, sizeof(buf), "the output ring holds %lld samples; one chunk releases up to %d (and at most 2^31 - 1 fit)",
               (long long)cap_out, win);
  }
  if (buf[0] && err) *err = buf;
  return buf[0] == 0;
}

StreamSched::StreamSched(int slots, int mode, int win, int par, int64_t cap_in, int64_t cap_out)
    : slots_(slots), mode_(mode), win_(win), par_(par), cap_in_(cap_in), cap_out_(cap_out), s_((size_t)std::max(slots, 0)) {}

bool StreamSched::fail(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  error = buf;
  return false;
}

bool StreamSched::slot_ok(int slot, const char* what) {
  if (slot < 0 || slot >= slots_) return fail("%s: slot %d does not exist (the session has %d)", what, slot, slots_);
  return true;
}

// Is chunk k of the slot due, and what is it?  (Back-pressure is the caller's.)
bool StreamSched::due(const Slot& s, int64_t k, Chunk* c) const {
  const int64_t W = win_, P = par_, L = s.fed;
  const bool closing = s.state == CLOSING;
  if (s.state != OPEN && !closing) return false;
  c->valid_end = L;
  if (mode_ == STREAM_OLA) {
    if (closing ? !(L > 0 && k <= (L + W - 1) / P) : L < k * P) return false;
    const bool last = closing && k == (L + W - 1) / P;
    c->start = k * P - W;
    c->len = (int)W;
    c->off = 0;
    c->consumed_after = std::max<int64_t>(0, (k + 1) * P - W);
    c->n0 = last ? k * P : c->consumed_after;                   // final_end: at close everything the last chunk touches is final
    c->release_end = last ? L : c->consumed_after;
    c->count = 0;
    return true;
  }
  const int64_t nch = (L + W - 1) / W, tail = L % W;
  if (closing ? k >= nch : L < (k + 1) * W + P) return false;
  c->n0 = k * W;
  c->consumed_after = std::max<int64_t>(0, (k + 1) * W - P);
  if (k == 0) {
    c->start = 0, c->len = (int)(W + P), c->off = 0, c->count = closing ? std::min(W, L) : W;
  } else if (closing && k == nch - 1) {
    c->start = k * W - P, c->len = (int)(P + (tail ? tail : W)), c->off = (int)P, c->count = tail ? tail : W;
  } else {
    c->start = k * W - P, c->len = (int)(W + 2 * P), c->off = (int)P, c->count = W;
  }
  c->release_end = c->n0 + c->count;
  return true;
}

bool StreamSched::open(int* slot) {
  for (int i = 0; i < slots_; ++i) {
    Slot& s = s_[(size_t)i];
    if (s.state == FREE || (s.state == CLOSED && s.popped == s.released)) {
      const int parity = s.parity;
      s = Slot();
      s.parity = parity;
      s.state = OPEN;
      s.next = mode_ == STREAM_OLA ? 1 : 0;
      *slot = i;
      return true;
    }
  }
  return fail("open: all %d slots are in use (a closed slot is free again once its output is popped)", slots_);
}

bool StreamSched::push(int n, const int* slots, const int64_t* counts, std::vector<StreamCopyRow>* rows) {
  rows->clear();
  for (int i = 0; i < n; ++i) {
    if (!slot_ok(slots[i], "push")) return false;
    const Slot& s = s_[(size_t)slots[i]];
    if (s.state != OPEN) return fail("push: slot %d is not open", slots[i]);
    if (counts[i] < 0) return fail("push: slot %d is given %lld samples", slots[i], (long long)counts[i]);
    for (int j = 0; j < i; ++j)
      if (slots[j] == slots[i]) return fail("push: slot %d is named twice", slots[i]);
    const int64_t room = cap_in_ - (s.fed - s.consumed);
    if (counts[i] > room)
      return fail("push: %lld samples would overrun the input ring of slot %d (room for %lld of %lld)", (long long)counts[i], slots[i],
                  (long long)room, (long long)cap_in_);
  }
  int64_t off = 0;
  for (int i = 0; i < n; ++i) {
    Slot& s = s_[(size_t)slots[i]];
    if (counts[i] > 0) rows->push_back(StreamCopyRow{slots[i], off, counts[i], s.fed % cap_in_});
    s.fed += counts[i];
    off += counts[i];
  }
  return true;
}

bool StreamSched::close(int slot) {
  if (!slot_ok(slot, "close")) return false;
  Slot& s = s_[(size_t)slot];
  if (s.state != OPEN) return fail("close: slot %d is not open", slot);
  s.state = CLOSING;
  for (const Item& it : group_)
    if (it.slot == slot) return true;   // put() finishes it
  Chunk c;
  if (!due(s, s.next, &c)) s.state = CLOSED;
  return true;
}

bool StreamSched::next(int max_rows, std::vector<StreamGatherRow>* rows, int* row_len) {
  rows->clear();
  *row_len = 0;
  if (!group_.empty()) return fail("next: the previous group of %d rows has not been put", (int)group_.size());
  if (max_rows < 1) return fail("next: max_rows = %d", max_rows);
  for (int i = 0; i < slots_ && (int)group_.size() < max_rows; ++i) {
    Slot& s = s_[(size_t)i];
    Chunk c;
    while ((int)group_.size() < max_rows && due(s, s.next, &c)) {
      if (c.release_end - s.popped > cap_out_) break;      // back-pressure: no room for what this chunk releases
      if (*row_len && c.len != *row_len) break;            // one row length per group
      *row_len = c.len;
      group_.push_back(Item{i, s.next, c});
      const int64_t pos = ((c.start % cap_in_) + cap_in_) % cap_in_;
      rows->push_back(StreamGatherRow{i, c.start, c.valid_end, pos});
      s.consumed = c.consumed_after;
      ++s.next;
    }
  }
  return true;
}

bool StreamSched::put(std::vector<StreamOlaRow>* ola, std::vector<StreamBoxRow>* box) {
  ola->clear();
  box->clear();
  if (group_.empty()) return fail("put: no group is outstanding (call next first)");
  for (size_t a = 0; a < group_.size();) {
    size_t b = a;
    while (b < group_.size() && group_[b].slot == group_[a].slot) ++b;
    Slot& s = s_[(size_t)group_[a].slot];
    const Item& first = group_[a];
    const Item& last = group_[b - 1];
    if (mode_ == STREAM_OLA) {
      StreamOlaRow r;
      r.slot = first.slot, r.row0 = (int)a, r.nk = (int)(b - a), r.parity = s.parity;
      r.k0 = first.k;
      r.span0 = std::max<int64_t>(0, first.c.start);
      r.span1 = last.k * par_;
      r.prior_end = (first.k - 1) * par_;
      r.final_end = last.c.n0;
      r.out_limit = last.c.release_end;
      ola->push_back(r);
      s.parity ^= 1;
    } else {
      for (size_t j = a; j < b; ++j)
        box->push_back(StreamBoxRow{group_[j].slot, (int)j, group_[j].c.off, group_[j].c.count, group_[j].c.n0});
    }
    s.released = std::max(s.released, last.c.release_end);
    Chunk c;
    if (s.state == CLOSING && !due(s, s.next, &c)) s.state = CLOSED;
    a = b;
  }
  group_.clear();
  return true;
}

bool StreamSched::available(int slot, int64_t* n) const {
  if (slot < 0 || slot >= slots_) return false;
  *n = s_[(size_t)slot].released - s_[(size_t)slot].popped;
  return true;
}

bool StreamSched::room(int slot, int64_t* n) const {
  if (slot < 0 || slot >= slots_) return false;
  const Slot& s = s_[(size_t)slot];
  *n = s.state == OPEN ? cap_in_ - (s.fed - s.consumed) : 0;
  return true;
}

bool StreamSched::state(int slot, int64_t* fed, int64_t* released) const {
  if (slot < 0 || slot >= slots_) return false;
  *fed = s_[(size_t)slot].fed;
  *released = s_[(size_t)slot].released;
  return true;
}

bool StreamSched::pop(int n, const int* slots, const int64_t* max_counts, std::vector<StreamCopyRow>* rows, int64_t* counts_out) {
  rows->clear();
  for (int i = 0; i < n; ++i) {
    if (!slot_ok(slots[i], "pop")) return false;
    if (s_[(size_t)slots[i]].state == FREE) return fail("pop: slot %d has never been opened", slots[i]);
    if (max_counts[i] < 0) return fail("pop: slot %d is asked for %lld samples", slots[i], (long long)max_counts[i]);
    for (int j = 0; j < i; ++j)
      if (slots[j] == slots[i]) return fail("pop: slot %d is named twice", slots[i]);
  }
  int64_t off = 0;
  for (int i = 0; i < n; ++i) {
    Slot& s = s_[(size_t)slots[i]];
    const int64_t c = std::min(max_counts[i], s.released - s.popped);
    counts_out[i] = c;
    if (c > 0) rows->push_back(StreamCopyRow{slots[i], off, c, s.popped % cap_out_});
    s.popped += c;
    off += c;
  }
  return true;
}

}  // namespace vfx
