// guide_rescue.hip -- test-only translation unit (tests/test_gpu_guide_rescue.py): the product's two small kernels of the guide
// rescue (k_rescue_select and k_rescue_merge of dynamont_amd/csrc/guide_rescue.hip, launched through launch_rescue_select /
// launch_rescue_merge exactly as enqueue_job launches them) on tables and buffers the HOST hands in.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../dynamont_amd/csrc/guide_rescue.hip"  // (this directory has a file of the same name)

using dynk::ReadDesc;
using dynk::ReadState;

namespace {
struct Dev {  // device allocations of one run, freed together
  std::vector<void*> ptrs;
  hipError_t alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes ? bytes : 4);
    if (e == hipSuccess) ptrs.push_back(*p);
    return e;
  }
  ~Dev() {
    for (void* p : ptrs) (void)hipFree(p);
  }
};
#define GR_TRY(expr)                      \
  do {                                    \
    const hipError_t _e = (expr);         \
    if (_e != hipSuccess) return (int)_e; \
  } while (0)
}  // namespace

// k_rescue_select over n_desc descriptors (T, N, read) and n_reads reads (status, low, high). code[n_reads] and list[n_desc]
// come back as the device holds them (list filled with 0xFFFFFFFF beforehand), *n_list likewise. Returns 0, a hipError_t, or
// -1 for a bad argument.
extern "C" int gr_select_run(int n_desc, const uint32_t* T, const uint32_t* N, const uint32_t* read, int n_reads, const int32_t* status,
                             const uint32_t* low, const uint32_t* high, uint32_t min_margin, uint32_t max_T, uint8_t* code,
                             uint32_t* list, uint32_t* n_list) {
  if (n_desc < 0 || n_reads < 1 || n_desc > (1 << 20) || n_reads > (1 << 20)) return -1;
  for (int k = 0; k < n_desc; ++k)
    if (read[k] >= (uint32_t)n_reads) return -1;  // everything the kernel indexes is inside what was handed in
  std::vector<ReadDesc> descs((size_t)n_desc);
  for (int k = 0; k < n_desc; ++k) {
    ReadDesc d{};
    d.T = T[k];
    d.N = N[k];
    d.read = read[k];
    d.sig_off = d.par_off = d.path_off = d.seg_off = 0x7fffffffffffff00ull;  // never read by the kernel
    descs[(size_t)k] = d;
  }
  std::vector<ReadState> st((size_t)n_reads);
  for (int i = 0; i < n_reads; ++i) st[(size_t)i] = ReadState{0.0, 0.0, status[i], 0u};
  std::vector<uint32_t> filled((size_t)n_desc + 1, 0xffffffffu);
  Dev dev;
  void *d_descs, *d_st, *d_low, *d_high, *d_code, *d_list, *d_len;
  GR_TRY(dev.alloc(&d_descs, descs.size() * sizeof(ReadDesc)));
  GR_TRY(dev.alloc(&d_st, st.size() * sizeof(ReadState)));
  GR_TRY(dev.alloc(&d_low, (size_t)n_reads * 4));
  GR_TRY(dev.alloc(&d_high, (size_t)n_reads * 4));
  GR_TRY(dev.alloc(&d_code, (size_t)n_reads));
  GR_TRY(dev.alloc(&d_list, ((size_t)n_desc + 1) * 4));
  GR_TRY(dev.alloc(&d_len, 256));
  if (n_desc) GR_TRY(hipMemcpy(d_descs, descs.data(), descs.size() * sizeof(ReadDesc), hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_st, st.data(), st.size() * sizeof(ReadState), hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_low, low, (size_t)n_reads * 4, hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_high, high, (size_t)n_reads * 4, hipMemcpyHostToDevice));
  GR_TRY(hipMemset(d_code, 0, (size_t)n_reads));
  GR_TRY(hipMemcpy(d_list, filled.data(), filled.size() * 4, hipMemcpyHostToDevice));
  GR_TRY(hipMemset(d_len, 0xff, 256));
  dynk::RescueSelect r{};
  r.descs = static_cast<const ReadDesc*>(d_descs);
  r.n_reads = n_desc;
  r.st = static_cast<const ReadState*>(d_st);
  r.low = static_cast<const uint32_t*>(d_low);
  r.high = static_cast<const uint32_t*>(d_high);
  r.min_margin = min_margin;
  r.max_T = max_T;
  r.code = static_cast<uint8_t*>(d_code);
  r.list = static_cast<uint32_t*>(d_list);
  r.n_list = static_cast<uint32_t*>(d_len);
  GR_TRY(dynk::launch_rescue_select(r, nullptr));
  GR_TRY(hipDeviceSynchronize());
  GR_TRY(hipMemcpy(code, d_code, (size_t)n_reads, hipMemcpyDeviceToHost));
  if (n_desc) GR_TRY(hipMemcpy(list, d_list, (size_t)n_desc * 4, hipMemcpyDeviceToHost));
  GR_TRY(hipMemcpy(n_list, d_len, 4, hipMemcpyDeviceToHost));
  return 0;
}

// k_rescue_merge over n_desc descriptors (T, N, read, path_off, seg_off) of which list[0 .. n_list) are listed. The plain
// buffers (status / Z / n_segments per read, pp / pathn over n_rows path rows, segrow over n_seg segment rows, code / rounds /
// converged per read) are updated in place; the rescue's (the *_in arrays) are read only.
extern "C" int gr_merge_run(int n_desc, const uint32_t* T, const uint32_t* N, const uint32_t* read, const uint64_t* path_off,
                            const uint64_t* seg_off, int n_list, const uint32_t* list, int n_reads, uint64_t n_rows, uint64_t n_seg,
                            const int32_t* status_in, const double* z_in, const double* pp_in, const uint32_t* pathn_in,
                            const uint32_t* segrow_in, int32_t* status, double* z, uint32_t* n_segments, double* pp, uint32_t* pathn,
                            uint32_t* segrow, uint8_t* code, uint32_t* rounds, uint32_t* converged, int single) {
  if (n_desc < 1 || n_reads < 1 || n_list < 0 || n_list > n_desc || n_rows < 1 || n_seg < 1) return -1;
  for (int k = 0; k < n_desc; ++k) {  // everything the kernel indexes is inside what was handed in
    if (read[k] >= (uint32_t)n_reads || T[k] < 1 || N[k] < 1) return -1;
    if (path_off[k] > n_rows || T[k] > n_rows - path_off[k]) return -1;
    if (seg_off[k] > n_seg || (uint64_t)(N[k] - 1) > n_seg - seg_off[k]) return -1;
  }
  for (int k = 0; k < n_list; ++k)
    if (list[k] >= (uint32_t)n_desc) return -1;
  std::vector<ReadDesc> descs((size_t)n_desc);
  for (int k = 0; k < n_desc; ++k) {
    ReadDesc d{};
    d.T = T[k];
    d.N = N[k];
    d.read = read[k];
    d.path_off = path_off[k];
    d.seg_off = seg_off[k];
    d.sig_off = d.par_off = 0x7fffffffffffff00ull;  // never read by the kernel
    descs[(size_t)k] = d;
  }
  std::vector<ReadState> st_in((size_t)n_reads), st((size_t)n_reads);
  for (int i = 0; i < n_reads; ++i) {
    st_in[(size_t)i] = ReadState{z_in[i], z_in[i], status_in[i], status_in[i] ? 0u : 1u};
    st[(size_t)i] = ReadState{z[i], z[i], status[i], n_segments[i]};
  }
  std::vector<uint32_t> lst((size_t)n_desc, 0xffffffffu);
  for (int k = 0; k < n_list; ++k) lst[(size_t)k] = list[k];
  const uint32_t len = (uint32_t)n_list;
  Dev dev;
  void *d_descs, *d_list, *d_len, *d_st_in, *d_pp_in, *d_pn_in, *d_sr_in, *d_st, *d_pp, *d_pn, *d_sr, *d_code, *d_rounds, *d_conv;
  GR_TRY(dev.alloc(&d_descs, descs.size() * sizeof(ReadDesc)));
  GR_TRY(dev.alloc(&d_list, lst.size() * 4));
  GR_TRY(dev.alloc(&d_len, 256));
  GR_TRY(dev.alloc(&d_st_in, st_in.size() * sizeof(ReadState)));
  GR_TRY(dev.alloc(&d_pp_in, n_rows * 8));
  GR_TRY(dev.alloc(&d_pn_in, n_rows * 4));
  GR_TRY(dev.alloc(&d_sr_in, n_seg * 4));
  GR_TRY(dev.alloc(&d_st, st.size() * sizeof(ReadState)));
  GR_TRY(dev.alloc(&d_pp, n_rows * 8));
  GR_TRY(dev.alloc(&d_pn, n_rows * 4));
  GR_TRY(dev.alloc(&d_sr, n_seg * 4));
  GR_TRY(dev.alloc(&d_code, (size_t)n_reads));
  GR_TRY(dev.alloc(&d_rounds, (size_t)n_reads * 4));
  GR_TRY(dev.alloc(&d_conv, (size_t)n_reads * 4));
  GR_TRY(hipMemcpy(d_descs, descs.data(), descs.size() * sizeof(ReadDesc), hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_list, lst.data(), lst.size() * 4, hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_len, &len, 4, hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_st_in, st_in.data(), st_in.size() * sizeof(ReadState), hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_pp_in, pp_in, n_rows * 8, hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_pn_in, pathn_in, n_rows * 4, hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_sr_in, segrow_in, n_seg * 4, hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_st, st.data(), st.size() * sizeof(ReadState), hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_pp, pp, n_rows * 8, hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_pn, pathn, n_rows * 4, hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_sr, segrow, n_seg * 4, hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_code, code, (size_t)n_reads, hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_rounds, rounds, (size_t)n_reads * 4, hipMemcpyHostToDevice));
  GR_TRY(hipMemcpy(d_conv, converged, (size_t)n_reads * 4, hipMemcpyHostToDevice));
  dynk::RescueMerge m{};
  m.descs = static_cast<const ReadDesc*>(d_descs);
  m.n_reads = n_desc;
  m.list = static_cast<const uint32_t*>(d_list);
  m.n_list = static_cast<const uint32_t*>(d_len);
  m.st_in = static_cast<const ReadState*>(d_st_in);
  m.pp_in = static_cast<const double*>(d_pp_in);
  m.pathn_in = static_cast<const uint32_t*>(d_pn_in);
  m.segrow_in = static_cast<const uint32_t*>(d_sr_in);
  m.st = static_cast<ReadState*>(d_st);
  m.pp = static_cast<double*>(d_pp);
  m.pathn = static_cast<uint32_t*>(d_pn);
  m.segrow = static_cast<uint32_t*>(d_sr);
  m.code = static_cast<uint8_t*>(d_code);
  m.rounds = static_cast<uint32_t*>(d_rounds);
  m.converged = static_cast<uint32_t*>(d_conv);
  m.single = single;
  GR_TRY(dynk::launch_rescue_merge(m, nullptr));
  GR_TRY(hipDeviceSynchronize());
  GR_TRY(hipMemcpy(st.data(), d_st, st.size() * sizeof(ReadState), hipMemcpyDeviceToHost));
  for (int i = 0; i < n_reads; ++i) {
    status[i] = st[(size_t)i].status;
    z[i] = st[(size_t)i].Zb;
    n_segments[i] = st[(size_t)i].n_segments;
  }
  GR_TRY(hipMemcpy(pp, d_pp, n_rows * 8, hipMemcpyDeviceToHost));
  GR_TRY(hipMemcpy(pathn, d_pn, n_rows * 4, hipMemcpyDeviceToHost));
  GR_TRY(hipMemcpy(segrow, d_sr, n_seg * 4, hipMemcpyDeviceToHost));
  GR_TRY(hipMemcpy(code, d_code, (size_t)n_reads, hipMemcpyDeviceToHost));
  GR_TRY(hipMemcpy(rounds, d_rounds, (size_t)n_reads * 4, hipMemcpyDeviceToHost));
  GR_TRY(hipMemcpy(converged, d_conv, (size_t)n_reads * 4, hipMemcpyDeviceToHost));
  return 0;
}
