// exp_rate_probe.hip -- the issue cost of v_exp_f32 beside v_mul_f32 and v_add_f32 on gfx950, in shader cycles per
// instruction and SIMD at 1, 2, 4 and 8 waves per SIMD (the method of valu_microbench2.hip: eight independent chains,
// s_memtime around the loop).  tools/emd_time.py reads the last line for its issue floor.
//   hipcc --offload-arch=gfx950 -O3 tools/exp_rate_probe.hip -o tools/exp_rate_probe && tools/exp_rate_probe
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <vector>

#define REP8(x) x x x x x x x x
#define OPS8(fmt)                                                                                              \
  REP8(asm volatile(fmt(0) fmt(1) fmt(2) fmt(3) fmt(4) fmt(5) fmt(6) fmt(7)                                    \
                    : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)           \
                    : "v"(c0));)
#define F_MUL(i) "v_mul_f32 %" #i ", %" #i ", %8\n"
#define F_ADD(i) "v_add_f32 %" #i ", %" #i ", %8\n"
#define F_EXP(i) "v_exp_f32 %" #i ", %" #i "\n"

template <int KIND>
__global__ __launch_bounds__(256) void probe(float* out, long long* cyc, int iters) {
  float a0 = threadIdx.x * -1e-3f, a1 = a0 - 1, a2 = a0 - 2, a3 = a0 - 3, a4 = a0 - 4, a5 = a0 - 5, a6 = a0 - 6, a7 = a0 - 7;
  const float c0 = 0.999f + threadIdx.x * 1e-6f;
  const long long t0 = __builtin_amdgcn_s_memtime();
  for (int i = 0; i < iters; ++i) {
    if (KIND == 0) { OPS8(F_MUL) }
    else if (KIND == 1) { OPS8(F_ADD) }
    else { OPS8(F_EXP) }
  }
  const long long t1 = __builtin_amdgcn_s_memtime();
  if ((threadIdx.x & 63) == 0) cyc[blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;
  out[blockIdx.x * 256 + threadIdx.x] = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
}

template <int KIND>
double run(const char* name, double (&per_inst)[4]) {
  printf("%-12s", name);
  int slot = 0;
  for (int w : {1, 2, 4, 8}) {
    const int blocks = 256 * w, iters = 2000;
    float* out;
    long long* cyc;
    if (hipMalloc(&out, sizeof(float) * blocks * 256) != hipSuccess || hipMalloc(&cyc, sizeof(long long) * blocks * 4) != hipSuccess) return -1;
    probe<KIND><<<blocks, 256>>>(out, cyc, 50);
    probe<KIND><<<blocks, 256>>>(out, cyc, iters);
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    std::vector<long long> h(blocks * 4);
    (void)hipMemcpy(h.data(), cyc, sizeof(long long) * blocks * 4, hipMemcpyDeviceToHost);
    std::sort(h.begin(), h.end());
    per_inst[slot] = (double)h[h.size() / 2] / ((double)iters * 64) / w;
    printf("  w%d: %5.2f cyc/inst/SIMD", w, per_inst[slot]);
    ++slot;
    (void)hipFree(out);
    (void)hipFree(cyc);
  }
  printf("\n");
  return 0;
}

int main() {
  double mul[4], add[4], ex[4];
  if (run<0>("v_mul_f32", mul) < 0 || run<1>("v_add_f32", add) < 0 || run<2>("v_exp_f32", ex) < 0) return 1;
  printf("v_exp_f32 over v_mul_f32 at 1, 2, 4, 8 waves per SIMD: %.2f %.2f %.2f %.2f\n", ex[0] / mul[0], ex[1] / mul[1],
         ex[2] / mul[2], ex[3] / mul[3]);
  return 0;
}
