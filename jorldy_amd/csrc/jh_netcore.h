// What a network object over flat fp32 buckets needs that is not its architecture (jh_rbnet, jh_iqnnet, jh_acnet / jh_sacnet; jh_pponet takes
// ownership and the workspace only): the allocations it owns, the tile engine's workspace, the optimizer's device blocks, the segment table.
#pragma once
#include "jh_fused.h"
#include "jh_tgemm.h"

struct NetCore {
  jh_ctx* ctx = nullptr;
  std::vector<void*> owned;   // hipMalloc
  std::vector<void*> mapped;  // hipHostMalloc(hipHostMallocMapped)
  TGemmWorkspace tg;
  float* norm_partial = nullptr;  // 256 floats: the global-norm clip's per-workgroup sums of squares (optim_init; one per core, the optimizers run in turn)
};

// `who` names the object in the error string.  Whatever these hand out is the core's from then on -- also when a later step fails.
int core_alloc(NetCore* c, const char* who, void** out, size_t bytes, bool zero);                       // 0 bytes: 16
int core_alloc_mapped(NetCore* c, const char* who, void** host_out, void** dev_out, size_t bytes);      // pinned host memory + its device alias
int core_workspace(NetCore* c, const char* who, size_t ws_floats, int cnt_slots);                       // split-K partials (ws_floats * 4 bytes) + zeroed arrival counters
int core_drain(void);     // end of a create: the memsets and copies above have executed before any stream of the caller's reads what they wrote
void core_release(NetCore* c);  // set the device, let it drain, free everything; the core is empty again
static inline int core_tgemm(const NetCore* c, const char* name, TGemm* probs, int n, hipStream_t st) { return jh_tgemm_launch(c->tg, name, probs, n, st); }

// One optimizer over flat buckets (jh_flat_adam_step / jh_rb_optim_kernel): the hyper block, filled with torch.optim.Adam's defaults at
// lr 1e-3, and the zeroed ticket of "the last workgroup stores the new step" -- 2048 bytes: eight counters 128 bytes apart, one per residue
// of the workgroup index mod 8, and at byte 1024 the one on top of them.
struct FlatOptim {
  float* hyper = nullptr;
  unsigned* ticket = nullptr;
};
int optim_init(NetCore* c, const char* who, FlatOptim* o);

// ---- segment table: parameter tensors [rows][cols] packed one after the other, every offset a multiple of 4 floats (16-byte accesses)
static inline int64_t up4(int64_t x) { return (x + 3) & ~(int64_t)3; }
// offsets of segments [first, last) from 0 -> the floats they take
static inline int64_t seg_pack(const int* rows, const int* cols, int first, int last, int64_t* off) {
  int64_t o = 0;
  for (int i = first; i < last; ++i) {
    off[i] = o;
    o = up4(o + (int64_t)rows[i] * cols[i]);
  }
  return o;
}
// segment i of an object that keeps its table as seg_off / seg_rows / seg_cols [count]
template <typename Net>
static inline int seg_query(const Net* n, int count, int32_t i, int64_t* offset, int32_t* rows, int32_t* cols) {
  JH_ARG(n && i >= 0 && i < count && offset && rows && cols);
  *offset = n->seg_off[i]; *rows = n->seg_rows[i]; *cols = n->seg_cols[i];
  return JH_OK;
}
