// Stand-alone driver of the streaming scheduler (voicefixer_main_amd/csrc/stream_sched.cpp) for test_stream_sessions_host.py: it
// replays a list of calls and prints the schedule the scheduler answers with, one line per call, in the format tests/stream_ref.py
// logs its own.  Host code only; the test builds it with -fsanitize=address,undefined and runs it as a program of its own.
//
//   S slots mode win par cap_in cap_out     a new session (first line)
//   O                                       open
//   P n slot count slot count ...           push
//   C slot                                  close
//   N max_rows                              next, and put when rows came
//   G n slot slot ...                       pop all that is available of the slots
//   R slot                                  state
#include <cstdio>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "stream_sched.h"

using namespace vfx;

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s OPS_FILE\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  std::string line;
  std::unique_ptr<StreamSched> sc;
  int mode = 0;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    char op = 0;
    ls >> op;
    if (op == 'S') {
      int slots, win, par;
      long long ci, co;
      ls >> slots >> mode >> win >> par >> ci >> co;
      std::string why;
      if (!StreamSched::check_geometry(slots, mode, win, par, ci, co, &why)) {
        printf("refused: %s\n", why.c_str());
        return 1;
      }
      sc.reset(new StreamSched(slots, mode, win, par, ci, co));
      continue;
    }
    if (!sc) return 2;
    if (op == 'O') {
      int slot = -1;
      if (sc->open(&slot))
        printf("open %d\n", slot);
      else
        printf("open refused\n");
    } else if (op == 'P' || op == 'G') {
      int n = 0;
      ls >> n;
      std::vector<int> slots((size_t)n);
      std::vector<int64_t> counts((size_t)n, (int64_t)1 << 40), got((size_t)n);
      for (int i = 0; i < n; ++i) {
        ls >> slots[(size_t)i];
        if (op == 'P') {
          long long c;
          ls >> c;
          counts[(size_t)i] = c;
        }
      }
      std::vector<StreamCopyRow> rows;
      const bool ok = op == 'P' ? sc->push(n, slots.data(), counts.data(), &rows) : sc->pop(n, slots.data(), counts.data(), &rows, got.data());
      printf("%s", op == 'P' ? "push" : "pop");
      if (!ok) printf(" refused");
      for (const StreamCopyRow& r : rows) printf(" %d:%lld:%lld:%lld", r.slot, (long long)r.off, (long long)r.count, (long long)r.pos);
      printf("\n");
    } else if (op == 'C') {
      int slot = -1;
      ls >> slot;
      printf(sc->close(slot) ? "close %d\n" : "close refused %d\n", slot);
    } else if (op == 'N') {
      int max_rows = 0, row_len = 0;
      ls >> max_rows;
      std::vector<StreamGatherRow> rows;
      if (!sc->next(max_rows, &rows, &row_len)) {
        printf("next refused\n");
        continue;
      }
      if (rows.empty()) {
        printf("next 0\n");
        continue;
      }
      printf("next %d", row_len);
      for (const StreamGatherRow& r : rows) printf(" %d:%lld:%lld:%lld", r.slot, (long long)r.start, (long long)r.valid_end, (long long)r.pos);
      printf("\n");
      std::vector<StreamOlaRow> ola;
      std::vector<StreamBoxRow> box;
      if (!sc->put(&ola, &box)) {
        printf("put refused\n");
        continue;
      }
      printf("put");
      for (const StreamOlaRow& r : ola)
        printf(" %d:%d:%d:%lld:%lld:%lld:%lld:%lld", r.slot, r.row0, r.nk, (long long)r.k0, (long long)r.span0, (long long)r.span1,
               (long long)r.final_end, (long long)r.out_limit);
      for (const StreamBoxRow& r : box) printf(" %d:%d:%d:%lld:%lld", r.slot, r.row, r.off, (long long)r.count, (long long)r.n0);
      printf("\n");
    } else if (op == 'R') {
      int slot = -1;
      int64_t fed = 0, released = 0, avail = 0, room = 0;
      ls >> slot;
      if (sc->state(slot, &fed, &released) && sc->available(slot, &avail) && sc->room(slot, &room))
        printf("state %d %lld %lld %lld %lld\n", slot, (long long)fed, (long long)released, (long long)avail, (long long)room);
      else
        printf("state refused\n");
    }
  }
  return 0;
}
