// Launch-time record of the log map kernels: lv_so3_log_fwd / _bwd and
// lv_so3_rel_log_fwd / _bwd at n samples, beside an empty kernel of the same grid.  Each figure
// is the time between two device events around K back-to-back launches, over K; the variants
// alternate inside every round and the median [min-max] over the rounds is printed.
//   hipcc -O3 --offload-arch=gfx950 -I include tools/kbench_so3_log.hip \
//       -L lie-vae_amd/lie_vae -llievae_hip -Wl,-rpath,'$ORIGIN/../lie-vae_amd/lie_vae' \
//       -o tools/kbench_so3_log
//   tools/kbench_so3_log [n ...]        (default 4096 65536)
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

// Haar rotations from normalised Gaussian quaternions, row-major
static void fill_rotations(std::vector<float>& R, int64_t n, unsigned seed) {
  std::mt19937 gen(seed);
  std::normal_distribution<double> nd;
  R.resize(n * 9);
  for (int64_t i = 0; i < n; ++i) {
    double q[4], s = 0;
    for (double& x : q) { x = nd(gen); s += x * x; }
    s = std::sqrt(s);
    const double x = q[0] / s, y = q[1] / s, z = q[2] / s, w = q[3] / s;
    const double r[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                         2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)};
    for (int k = 0; k < 9; ++k) R[i * 9 + k] = (float)r[k];
  }
}

int main(int argc, char** argv) {
  std::vector<int64_t> sizes;
  for (int i = 1; i < argc; ++i) sizes.push_back(atoll(argv[i]));
  if (sizes.empty()) sizes = {4096, 65536};
  const int K = 200, rounds = 21, ns = 4;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int64_t n : sizes) {
    if (n <= 0 || n % ns) { printf("n must be a positive multiple of %d\n", ns); return 1; }
    const int64_t B = n / ns;  // rel_log: ns samples of B means, n rotations in all
    std::vector<float> hR, hmu, hg(n * 3);
    fill_rotations(hR, n, 1);
    fill_rotations(hmu, B, 2);
    std::mt19937 gen(3);
    std::normal_distribution<float> nd;
    for (float& x : hg) x = nd(gen);
    float *R, *mu, *gv, *v, *gR, *gmu;
    CK(hipMalloc(&R, n * 36)); CK(hipMalloc(&mu, B * 36)); CK(hipMalloc(&gv, n * 12));
    CK(hipMalloc(&v, n * 12)); CK(hipMalloc(&gR, n * 36)); CK(hipMalloc(&gmu, B * 36));
    CK(hipMemcpy(R, hR.data(), n * 36, hipMemcpyHostToDevice));
    CK(hipMemcpy(mu, hmu.data(), B * 36, hipMemcpyHostToDevice));
    CK(hipMemcpy(gv, hg.data(), n * 12, hipMemcpyHostToDevice));
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 65536);
    const unsigned grid_b = (unsigned)std::min<int64_t>((B + 255) / 256, 65536);
    std::vector<std::pair<std::string, std::function<void()>>> variants = {
        {"empty, grid of n", [&] { hipLaunchKernelGGL(empty_k, dim3(grid), dim3(256), 0, 0, n); }},
        {"empty, grid of B", [&] { hipLaunchKernelGGL(empty_k, dim3(grid_b), dim3(256), 0, 0, B); }},
        {"so3_log_fwd", [&] { LV(lv_so3_log_fwd(R, v, n, nullptr)); }},
        {"so3_log_bwd", [&] { LV(lv_so3_log_bwd(R, gv, gR, n, nullptr)); }},
        {"so3_rel_log_fwd", [&] { LV(lv_so3_rel_log_fwd(mu, R, v, ns, B, nullptr)); }},
        {"so3_rel_log_bwd", [&] { LV(lv_so3_rel_log_bwd(mu, R, gv, gmu, gR, ns, B, nullptr)); }},
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
    printf("n = %lld (rel_log: ns = %d, B = %lld; grids %u and %u blocks of 256), %d launches x %d rounds, us per launch\n",
           (long long)n, ns, (long long)B, grid, grid_b, K, rounds);
    for (size_t k = 0; k < variants.size(); ++k) {
      std::sort(us[k].begin(), us[k].end());
      printf("  %-18s %7.2f [%.2f-%.2f]\n", variants[k].first.c_str(), us[k][rounds / 2], us[k].front(), us[k].back());
    }
    fflush(stdout);
    CK(hipFree(R)); CK(hipFree(mu)); CK(hipFree(gv)); CK(hipFree(v)); CK(hipFree(gR)); CK(hipFree(gmu));
  }
  return 0;
}
