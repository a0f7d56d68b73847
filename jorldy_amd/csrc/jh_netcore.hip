// The network objects' core (jh_netcore.h): owned allocations, workspace, optimizer blocks, and the hyper block's upload.
#include "jh_netcore.h"

int core_alloc(NetCore* c, const char* who, void** out, size_t bytes, bool zero) {
  if (bytes == 0) bytes = 16;
  hipError_t e = hipMalloc(out, bytes);
  if (e != hipSuccess) return jh_fail(JH_ERR_NOMEM, "%s: hipMalloc(%zu) failed: %s", who, bytes, hipGetErrorString(e));
  c->owned.push_back(*out);
  if (zero) JH_HIP(hipMemset(*out, 0, bytes));
  return JH_OK;
}

int core_alloc_mapped(NetCore* c, const char* who, void** host_out, void** dev_out, size_t bytes) {
  hipError_t e = hipHostMalloc(host_out, bytes, hipHostMallocMapped);
  if (e != hipSuccess) return jh_fail(JH_ERR_NOMEM, "%s: hipHostMalloc(%zu) failed: %s", who, bytes, hipGetErrorString(e));
  c->mapped.push_back(*host_out);
  JH_HIP(hipHostGetDevicePointer(dev_out, *host_out, 0));
  return JH_OK;
}

int core_workspace(NetCore* c, const char* who, size_t ws_floats, int cnt_slots) {
  int rc = core_alloc(c, who, (void**)&c->tg.ws, sizeof(float) * ws_floats, false);
  if (rc) return rc;
  c->tg.ws_floats = ws_floats;
  c->tg.cnt_slots = cnt_slots;
  return core_alloc(c, who, (void**)&c->tg.cnt, sizeof(unsigned) * (size_t)cnt_slots * kTgemmCntStride, true);
}

int core_drain(void) {
  JH_HIP(hipDeviceSynchronize());
  return JH_OK;
}

void core_release(NetCore* c) {
  if (c->ctx) {
    (void)hipSetDevice(c->ctx->device);
    (void)hipDeviceSynchronize();
  }
  for (void* p : c->owned) (void)hipFree(p);
  for (void* p : c->mapped) (void)hipHostFree(p);
  c->owned.clear();
  c->mapped.clear();
}

int optim_init(NetCore* c, const char* who, FlatOptim* o) {
  int rc = core_alloc(c, who, (void**)&o->hyper, sizeof(float) * JH_HY_FLOATS, true);
  if (!rc) rc = core_alloc(c, who, (void**)&o->ticket, 2048, true);
  if (!rc && !c->norm_partial) rc = core_alloc(c, who, (void**)&c->norm_partial, sizeof(float) * 256, true);
  if (rc) return rc;
  float hy[JH_HY_FLOATS];
  jh_hyper_fill(hy, 1e-3, 0.9, 0.999, 1e-8, 0.0);
  JH_HIP(hipMemcpy(o->hyper, hy, sizeof(hy), hipMemcpyHostToDevice));
  return JH_OK;
}

int jh_hyper_upload(jh_ctx* ctx, float* d_hyper, double lr, double beta1, double beta2, double eps, int64_t step, int centered, hipStream_t st) {
  jh_pinned_slab* slab = nullptr;
  int rc = jh_ctx_slab(ctx, 64, &slab);
  if (rc) return rc;
  float* h = (float*)slab->host;
  jh_hyper_fill(h, lr, beta1, beta2, eps, (double)step);
  h[JH_HY_BC1] = centered ? 1.f : 0.f;
  JH_HIP(hipMemcpyAsync(d_hyper, slab->dev, JH_HY_FLOATS * sizeof(float), hipMemcpyDeviceToDevice, st));
  return jh_ctx_slab_release(ctx, slab, st);
}
int jh_hyper_upload_lr(jh_ctx* ctx, float* d_hyper, double lr, hipStream_t st) {
  jh_pinned_slab* slab = nullptr;
  int rc = jh_ctx_slab(ctx, 16, &slab);
  if (rc) return rc;
  *(float*)slab->host = (float)lr;
  JH_HIP(hipMemcpyAsync(d_hyper, slab->dev, sizeof(float), hipMemcpyDeviceToDevice, st));
  return jh_ctx_slab_release(ctx, slab, st);
}
