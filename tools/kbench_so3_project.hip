// Launch-time record of the SO(3) projection kernels: lv_so3_project_fwd / _bwd
// and their fp64 twins at n matrices, beside an empty kernel of the same grid, the fp64
// Gram-Schmidt map lv_s2s2_fwd_f64 / _bwd_f64 (the other projection-like mean map) and one
// lv_so3_moment (ns = 4, both launches).  Each figure is the time between two device events
// around K back-to-back launches, over K; the variants alternate inside every round and the
// median [min-max] over the rounds is printed.
//   hipcc -O3 --offload-arch=gfx950 -I include tools/kbench_so3_project.hip \
//       -L lie-vae_amd/lie_vae -llievae_hip -Wl,-rpath,'$ORIGIN/../lie-vae_amd/lie_vae' \
//       -o tools/kbench_so3_project
//   tools/kbench_so3_project [n ...]        (default 512 65536)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <string>
#include <vector>
#include "lievae.h"
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e)); exit(1);} } while (0)
#define LV(x) do { int rc = (x); if (rc != 0) { printf("%s:%d rc %d: %s\n", __FILE__, __LINE__, rc, lv_last_error()); exit(1);} } while (0)

__global__ void empty_k(int64_t n) {}

int main(int argc, char** argv) {
  std::vector<int64_t> sizes;
  for (int i = 1; i < argc; ++i) sizes.push_back(atoll(argv[i]));
  if (sizes.empty()) sizes = {512, 65536};
  const int K = 200, rounds = 21, ns = 4;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int64_t n : sizes) {
    if (n <= 0) { printf("n must be positive\n"); return 1; }
    // Gaussian 3x3 matrices (the head's raw output) and Gaussian upstream gradients
    std::mt19937 gen(1);
    std::normal_distribution<double> nd;
    std::vector<float> hM(n * 9), hg(n * 9);
    std::vector<double> hMd(n * 9), hgd(n * 9);
    for (int64_t i = 0; i < n * 9; ++i) { hMd[i] = nd(gen); hM[i] = (float)hMd[i]; }
    for (int64_t i = 0; i < n * 9; ++i) { hgd[i] = nd(gen); hg[i] = (float)hgd[i]; }
    const double hC[36] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, -1, 0, 0, 0, -1,
                           -1, 0, 0, 0, 1, 0, 0, 0, -1, -1, 0, 0, 0, -1, 0, 0, 0, 1};
    float hCf[36];
    for (int k = 0; k < 36; ++k) hCf[k] = (float)hC[k];
    float *M, *g, *R, *gM, *C, *Rs;
    double *Md, *gd, *Rd, *gMd, *g1, *g2, *S, *wsum;
    void* ws;
    const size_t ws_bytes = lv_so3_moment_workspace(n, ns);
    CK(hipMalloc(&M, n * 36)); CK(hipMalloc(&g, n * 36)); CK(hipMalloc(&R, n * 36)); CK(hipMalloc(&gM, n * 36));
    CK(hipMalloc(&Md, n * 72)); CK(hipMalloc(&gd, n * 72)); CK(hipMalloc(&Rd, n * 72)); CK(hipMalloc(&gMd, n * 72));
    CK(hipMalloc(&g1, n * 24)); CK(hipMalloc(&g2, n * 24));
    CK(hipMalloc(&C, sizeof(hCf))); CK(hipMalloc(&Rs, sizeof(hCf)));
    CK(hipMalloc(&S, ns * 72)); CK(hipMalloc(&wsum, 8)); CK(hipMalloc(&ws, ws_bytes));
    CK(hipMemcpy(M, hM.data(), n * 36, hipMemcpyHostToDevice));
    CK(hipMemcpy(g, hg.data(), n * 36, hipMemcpyHostToDevice));
    CK(hipMemcpy(Md, hMd.data(), n * 72, hipMemcpyHostToDevice));
    CK(hipMemcpy(gd, hgd.data(), n * 72, hipMemcpyHostToDevice));
    CK(hipMemcpy(C, hCf, sizeof(hCf), hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 65536);
    // s2s2 reads two (n,3) vectors: the first two rows' worth of the fp64 matrices
    std::vector<std::pair<std::string, std::function<void()>>> variants = {
        {"empty, grid of n", [&] { hipLaunchKernelGGL(empty_k, dim3(grid), dim3(256), 0, 0, n); }},
        {"so3_project_fwd", [&] { LV(lv_so3_project_fwd(M, R, n, nullptr)); }},
        {"so3_project_bwd", [&] { LV(lv_so3_project_bwd(M, g, gM, n, nullptr)); }},
        {"so3_project_fwd_f64", [&] { LV(lv_so3_project_fwd_f64(Md, Rd, n, nullptr)); }},
        {"so3_project_bwd_f64", [&] { LV(lv_so3_project_bwd_f64(Md, gd, gMd, n, nullptr)); }},
        {"s2s2_fwd_f64", [&] { LV(lv_s2s2_fwd_f64(Md, Md + n * 3, Rd, n, nullptr)); }},
        {"s2s2_bwd_f64", [&] { LV(lv_s2s2_bwd_f64(Md, Md + n * 3, gd, g1, g2, n, nullptr)); }},
        {"so3_moment ns=4", [&] { LV(lv_so3_moment(R, M, nullptr, C, ns, LV_MOMENT_YT | LV_MOMENT_CT, S, wsum, Rs, n, ws, ws_bytes, nullptr)); }},
    };
    std::vector<std::vector<float>> us(variants.size());
    for (auto& kv : variants) kv.second();  // warm: code objects loaded
    CK(hipDeviceSynchronize());
    for (int r = 0; r < rounds; ++r)
      for (size_t k = 0; k < variants.size(); ++k) {
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < K; ++i) variants[k].second();
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        us[k].push_back(ms * 1e3f / K);
      }
    CK(hipGetLastError());
    printf("n = %lld (grid %u blocks of 256; moment: ns = %d, two launches), %d launches x %d rounds, us per launch\n",
           (long long)n, grid, ns, K, rounds);
    for (size_t k = 0; k < variants.size(); ++k) {
      std::sort(us[k].begin(), us[k].end());
      printf("  %-20s %7.2f [%.2f-%.2f]\n", variants[k].first.c_str(), us[k][rounds / 2], us[k].front(), us[k].back());
    }
    fflush(stdout);
    for (void* p : {(void*)M, (void*)g, (void*)R, (void*)gM, (void*)Md, (void*)gd, (void*)Rd, (void*)gMd,
                    (void*)g1, (void*)g2, (void*)C, (void*)Rs, (void*)S, (void*)wsum, ws})
      CK(hipFree(p));
  }
  return 0;
}
