// pkrate.hip -- issue cost of the packed 16-bit instructions k_sw16 / k_sw16h are made of (not part of libsmr_hip):
//   hipcc --offload-arch=gfx950 -O3 -o build/pkrate pkrate.hip && build/pkrate [iterations]
//
// One workgroup of 768 threads per CU = 3 waves per SIMD (k_sw16<19>'s occupancy), every wave runs `iterations` trips of a loop of
// 8 x UNROLL instructions of ONE kind in 8 independent streams (no instruction waits for the one before it), so what is measured is the
// SIMD's issue rate for that instruction, not its latency; S = 1 (one dependent chain per wave) is printed beside it for the latency.
// Per instruction: the HIP-event time of the launch, cycles per instruction and SIMD at the nominal shader clock (event time x clock /
// (3 waves x instructions per wave)), the cost relative to v_pk_add_i16 -- the number the kernels' instruction counts are weighed with --
// and the mean span of a wave in ticks of its own counter (__builtin_readcyclecounter; the rate of that counter is not the shader clock).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); exit(2); } } while (0)

enum { OP_PK_ADD_I16, OP_PK_MAX_I16, OP_PK_ADD_F16, OP_PK_MAXIMUM3_F16, OP_PERM_B32, OP_PK_SUB_U16_CLAMP, OP_N };
static const char* const OP_NAME[OP_N] = {"v_pk_add_i16", "v_pk_max_i16", "v_pk_add_f16", "v_pk_maximum3_f16", "v_perm_b32", "v_pk_sub_u16 clamp"};

template <int OP> __device__ __forceinline__ void one(uint32_t& x, uint32_t b, uint32_t c) {
  if (OP == OP_PK_ADD_I16) asm volatile("v_pk_add_i16 %0, %0, %1" : "+v"(x) : "v"(b));
  else if (OP == OP_PK_MAX_I16) asm volatile("v_pk_max_i16 %0, %0, %1" : "+v"(x) : "v"(b));
  else if (OP == OP_PK_ADD_F16) asm volatile("v_pk_add_f16 %0, %0, %1" : "+v"(x) : "v"(b));
  else if (OP == OP_PK_MAXIMUM3_F16) asm volatile("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c));
  else if (OP == OP_PERM_B32) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(x) : "v"(b), "v"(c));
  else asm volatile("v_pk_sub_u16 %0, %0, %1 clamp" : "+v"(x) : "v"(b));
}

#define UNROLL 8
// S = 8: eight streams; S = 1: every instruction takes the result of the one before it
template <int OP, int S>
__global__ void __launch_bounds__(768) k_rate(uint32_t iters, uint32_t b, uint32_t c, unsigned long long* __restrict__ span, uint32_t* __restrict__ sink) {
  uint32_t x[8];
#pragma unroll
  for (int i = 0; i < 8; i++) x[i] = threadIdx.x * 8u + (uint32_t)i;
  // (b and c in vector registers: the f16 values 1.0 | 1.0 and 0.0 for the f16 kinds keep every stream finite)
  const uint32_t vb = b + (threadIdx.x & 0u), vc = c + (threadIdx.x & 0u);
  const unsigned long long t0 = __builtin_readcyclecounter();
  for (uint32_t it = 0; it < iters; it++) {
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
#pragma unroll
      for (int i = 0; i < 8; i++) one<OP>(x[S == 1 ? 0 : i], vb, vc);
    }
  }
  const unsigned long long t1 = __builtin_readcyclecounter();
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) acc ^= x[i];
  if (acc == 0x12345u) sink[0] = acc;
  if ((threadIdx.x & 63u) == 0) span[blockIdx.x * 12u + (threadIdx.x >> 6)] = t1 - t0;
}

typedef void (*rate_fn)(uint32_t, uint32_t, uint32_t, unsigned long long*, uint32_t*);
template <int S> static rate_fn kernel_of(int op) {
  switch (op) {
    case OP_PK_ADD_I16: return k_rate<OP_PK_ADD_I16, S>;
    case OP_PK_MAX_I16: return k_rate<OP_PK_MAX_I16, S>;
    case OP_PK_ADD_F16: return k_rate<OP_PK_ADD_F16, S>;
    case OP_PK_MAXIMUM3_F16: return k_rate<OP_PK_MAXIMUM3_F16, S>;
    case OP_PERM_B32: return k_rate<OP_PERM_B32, S>;
    default: return k_rate<OP_PK_SUB_U16_CLAMP, S>;
  }
}

int main(int argc, char** argv) {
  const uint32_t iters = argc > 1 ? (uint32_t)atoi(argv[1]) : 20000u;
  hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, 0));
  const int n_cu = prop.multiProcessorCount;
  int clock_khz = 0, wall_khz = 0;
  CK(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeClockRate, 0));
  CK(hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, 0));
  unsigned long long* span = nullptr; uint32_t* sink = nullptr;
  const size_t n_span = (size_t)n_cu * 12;
  CK(hipMalloc((void**)&span, n_span * 8)); CK(hipMalloc((void**)&sink, 4));
  unsigned long long* h = (unsigned long long*)malloc(n_span * 8);
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  printf("# %s, %d CUs, shader clock %d kHz, s_memtime counter %d kHz; one workgroup of 12 waves per CU = 3 waves per SIMD; %u trips x %d instructions per wave\n",
         prop.name, n_cu, clock_khz, wall_khz, iters, 8 * UNROLL);
  printf("# cyc/inst/SIMD: event time x shader clock / (3 waves x instructions per wave) -- the clock under load may be below the nominal one, the column `rel` does not depend on it\n");
  printf("%-20s %8s %10s %14s %8s %14s\n", "instruction", "streams", "ms", "cyc/inst/SIMD", "rel", "memtime ticks");
  double base[2] = {0, 0};
  for (int s = 0; s < 2; s++) {
    for (int op = 0; op < OP_N; op++) {
      const rate_fn k = s == 0 ? kernel_of<8>(op) : kernel_of<1>(op);
      const bool f16 = op == OP_PK_ADD_F16 || op == OP_PK_MAXIMUM3_F16;
      // f16: x = max3(x, 1.0, 0.0) and x = x + 0.0 keep the values finite; the integer kinds take any pattern
      const uint32_t b = f16 ? (op == OP_PK_ADD_F16 ? 0u : 0x3C003C00u) : 0x00010001u, c = f16 ? 0u : 0x07060100u;
      float best = 1e30f; unsigned long long ticks = 0;
      for (int rep = 0; rep < 4; rep++) {                 // (the first is the warm-up)
        CK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k, dim3(n_cu), dim3(768), 0, 0, iters, b, c, span, sink);
        CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
        float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
        if (rep > 0 && ms < best) {
          best = ms;
          CK(hipMemcpy(h, span, n_span * 8, hipMemcpyDeviceToHost));
          unsigned long long sum = 0; for (size_t i = 0; i < n_span; i++) sum += h[i];
          ticks = sum / n_span;
        }
      }
      const double inst = (double)iters * 8 * UNROLL;
      const double cyc = (double)best * 1e-3 * (double)clock_khz * 1e3 / (3.0 * inst);
      if (op == OP_PK_ADD_I16) base[s] = cyc;
      printf("%-20s %8d %10.3f %14.3f %8.3f %14llu\n", OP_NAME[op], s == 0 ? 8 : 1, best, cyc, cyc / base[s], ticks);
      fflush(stdout);
    }
  }
  free(h); CK(hipFree(span)); CK(hipFree(sink));
  return 0;
}
