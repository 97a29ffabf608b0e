// guide_rescue_host.cpp -- test-only: the guide rescue's decision rule (rescue_decide of
// dynamont_amd/csrc/guide_rescue_kernels.hpp, the function k_rescue_select calls per descriptor) in a plain g++ build, walked over
// a descriptor table the way the kernel walks it: codes per read, the list of descriptor indices in descriptor order.
// tests/test_guide_rescue_host.py compares both with a Python restatement.
#define DYN_GUIDE_RESCUE_RULE_ONLY
#include "guide_rescue_kernels.hpp"

// descriptors k = 0 .. n_desc-1 (T, N, read); per-read status / low / high; code[] is cleared by the caller. Returns the list's
// length.
extern "C" int gr_host_select(int n_desc, const uint32_t* T, const uint32_t* N, const uint32_t* read, const int32_t* status,
                              const uint32_t* low, const uint32_t* high, uint32_t min_margin, uint32_t max_T, uint8_t* code,
                              uint32_t* list) {
  int n = 0;
  for (int k = 0; k < n_desc; ++k) {
    const uint32_t r = read[k];
    const uint8_t c = dynk::rescue_decide(status[r], N[k], T[k], low[r], high[r], min_margin, max_T);
    if (c) code[r] = c;
    if (c == 1) list[n++] = (uint32_t)k;
  }
  return n;
}
