// salu_rate.hip — issue rate of scalar instructions on one CU of gfx950 (MI355X), measured: ticks per scalar instruction per CU
// with the waves of 1, 2 or 4 of the CU's SIMDs issuing them and n = 1 .. 8 such waves per SIMD; the same with waves that run
// 4-cycle vector instructions on the SAME SIMDs (half of every CU's workgroups, chosen by their order of arrival on the CU and
// checked through the hardware ids); and the round trip v_cmp -> SGPR pair -> s_and_b64 -> s_cmp -> branch, taken and not taken.
// k_fast_wave executes as many scalar as vector instructions, and a CU has ONE scalar unit for its four SIMDs (DESIGN.md
// section 5); tools/microbench/valu_rate.hip is the vector side, and its ticks (s_memtime) are the ticks here.
// build + run: hipcc -O3 --offload-arch=gfx950 -Wno-unused-value -Wno-unused-result tools/microbench/salu_rate.hip -o /tmp/salu_rate && /tmp/salu_rate
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#define REP 64      // instructions per loop iteration (eight independent chains, eight times)
#define ITERS 1000
#define CU_KEYS (8 * 256)  // XCC id (3 bits) x HW_ID bits 8 .. 15 (CU, shader array, shader engine)

// eight copies of one scalar instruction on eight chains.  The chains and the constant operands are C variables under "s"
// constraints: the compiler keeps them in registers of its choice across the statements
#define S8(ins, tail) ins " %0, " tail(0) "\n" ins " %1, " tail(1) "\n" ins " %2, " tail(2) "\n" ins " %3, " tail(3) "\n" \
                      ins " %4, " tail(4) "\n" ins " %5, " tail(5) "\n" ins " %6, " tail(6) "\n" ins " %7, " tail(7)
#define T_SELF_K(i) "%" #i ", %8"   // dst = dst op k
#define T_K_SELF(i) "%8, %" #i      // dst = cond ? k : dst
#define T_K(i) "%8"                 // dst = op k
#define CH32 "+s"(d0), "+s"(d1), "+s"(d2), "+s"(d3), "+s"(d4), "+s"(d5), "+s"(d6), "+s"(d7)
#define CH64 "+s"(q0), "+s"(q1), "+s"(q2), "+s"(q3), "+s"(q4), "+s"(q5), "+s"(q6), "+s"(q7)
// one round trip: a compare writes an SGPR pair, a scalar AND cuts it, a scalar compare tests it, a branch follows (to the next
// instruction either way: taken when the compare holds in some lane)
#define TRIP "v_cmp_gt_u32_e64 %0, %3, %4\n s_and_b64 %1, %0, %2\n s_cmp_lg_u64 %1, 0\n s_cbranch_scc1 1f\n s_nop 0\n1:\n"

__device__ __forceinline__ uint32_t hwId() {  // bits 4..5 SIMD, 8..11 CU, 12 shader array, 13..15 shader engine
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v));
  return v;
}
__device__ __forceinline__ uint32_t xccId() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(v));
  return v;
}

// OP: 0 s_add_i32, 1 s_and_b64, 2 s_cselect_b32, 3 s_bcnt1_i32_b64, 4 s_mov_b64 exec, 5 round trip taken, 6 round trip not taken.
// Waves on a SIMD >= simds leave at once.  vmix != 0: every second workgroup TO ARRIVE ON A CU (a counter per CU) runs v_min_i32
// (4 ticks per wave64 instruction, valu_rate.hip), eight independent chains, on the same four SIMDs as the others' waves; vmix == 2:
// the others leave at once (the vector waves alone, for comparison).  where[wave] = XCC << 16 | HW_ID: the host checks the sharing.
template <int OP>
__global__ __launch_bounds__(256) void k(float* out, unsigned long long* cyc, int* role, uint32_t* where, int* arrivals, int iters,
                                         int simds, int vmix) {
  extern __shared__ uint32_t dummyLds[];
  __shared__ int order;
  if (iters < 0) dummyLds[threadIdx.x] = 1;
  const uint32_t hw = hwId(), xcc = xccId();
  if (threadIdx.x == 0) order = vmix ? atomicAdd(&arrivals[(xcc & 7u) * 256u + ((hw >> 8) & 0xffu)], 1) : 0;
  __syncthreads();
  const int wave = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;
  const bool vec = vmix && (order & 1);
  const bool idle = (int)((hw >> 4) & 3u) >= simds || (vmix == 2 && !vec);
  float a0 = threadIdx.x, a1 = a0 + 1, a2 = a0 + 2, a3 = a0 + 3, a4 = a0 + 4, a5 = a0 + 5, a6 = a0 + 6, a7 = a0 + 7;
  const float k1 = out[0];
  const uint32_t lo = OP == 5 ? 0u : 1u, hi = OP == 5 ? 1u : 0u;  // hi > lo: the compare holds, the branch is taken
  uint32_t d0 = 1, d1 = 2, d2 = 3, d3 = 4, d4 = 5, d5 = 6, d6 = 7, d7 = 8;
  unsigned long long q0 = ~0ull, q1 = ~0ull, q2 = ~0ull, q3 = ~0ull, q4 = ~0ull, q5 = ~0ull, q6 = ~0ull, q7 = ~0ull;
  const uint32_t three = 3u;
  const unsigned long long ones = ~0ull;
  unsigned long long t0 = 0, t1 = 0;
  if (!idle) {
    t0 = __builtin_amdgcn_s_memtime();
    if (vec) {
      for (int it = 0; it < iters; it++)
#pragma unroll
        for (int r = 0; r < REP / 8; r++)
          asm volatile("v_min_i32 %0, %0, %8\n v_min_i32 %1, %1, %8\n v_min_i32 %2, %2, %8\n v_min_i32 %3, %3, %8\n"
                       "v_min_i32 %4, %4, %8\n v_min_i32 %5, %5, %8\n v_min_i32 %6, %6, %8\n v_min_i32 %7, %7, %8"
                       : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7)
                       : "v"(k1));
    } else {
      for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int r = 0; r < REP / 8; r++) {
          if (OP == 0) asm volatile(S8("s_add_i32", T_SELF_K) : CH32 : "s"(three) : "scc");
          if (OP == 1) asm volatile(S8("s_and_b64", T_SELF_K) : CH64 : "s"(ones) : "scc");
          if (OP == 2) asm volatile(S8("s_cselect_b32", T_K_SELF) : CH32 : "s"(three) : "scc");
          if (OP == 3) asm volatile(S8("s_bcnt1_i32_b64", T_K) : CH32 : "s"(ones) : "scc");
          if (OP == 4)  // (exec stays all ones: every lane of the workgroup is active here)
            asm volatile("s_mov_b64 exec, %0\n s_mov_b64 exec, %0\n s_mov_b64 exec, %0\n s_mov_b64 exec, %0\n"
                         "s_mov_b64 exec, %0\n s_mov_b64 exec, %0\n s_mov_b64 exec, %0\n s_mov_b64 exec, %0" : : "s"(ones));
          if (OP >= 5) asm volatile(TRIP TRIP TRIP TRIP TRIP TRIP TRIP TRIP : "=&s"(q0), "=&s"(q1) : "s"(ones), "v"(hi), "v"(lo) : "scc");
        }
      }
    }
    t1 = __builtin_amdgcn_s_memtime();
  }
  out[2 + blockIdx.x * blockDim.x + threadIdx.x] =
      a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7 + (float)(d0 ^ d1 ^ d2 ^ d3 ^ d4 ^ d5 ^ d6 ^ d7) + (float)(uint32_t)(q0 ^ q1 ^ q2 ^ q3 ^ q4 ^ q5 ^ q6 ^ q7);
  if ((threadIdx.x & 63) == 0) {
    cyc[wave] = t1 - t0;
    role[wave] = idle ? 0 : vec ? 2 : 1;
    where[wave] = (xcc & 7u) << 16 | (hw & 0xff30u);
  }
}

static double median(std::vector<unsigned long long>& v) {
  std::sort(v.begin(), v.end());
  return (double)v[v.size() / 2];
}

template <int OP>
void run(const char* name, int simds, int vmix) {
  float* out; unsigned long long* cyc; int *role, *arrivals; uint32_t* where;
  const int maxBlocks = 256 * 8 * 4;
  hipMalloc(&out, (2 + (size_t)maxBlocks * 256) * 4); hipMemset(out, 0, 64);
  hipMalloc(&cyc, (size_t)maxBlocks * 4 * 8); hipMalloc(&role, (size_t)maxBlocks * 4 * 4); hipMalloc(&where, (size_t)maxBlocks * 4 * 4);
  hipMalloc(&arrivals, CU_KEYS * 4);
  printf("%-24s simds=%d %-11s", name, simds, vmix == 1 ? "+valu" : vmix == 2 ? "valu alone" : "");
  for (int n : {1, 2, 4, 8}) {  // co-resident 256-thread workgroups per CU = waves per SIMD, enforced through the LDS size
    if (vmix && n == 1) continue;
    const int lds = 160 * 1024 / n - 2048;  // (the kernel has four static bytes of its own)
    // without vector waves four rounds (most waves run in the steady state); with them ONE round, every workgroup resident from the
    // start, so that each SIMD holds n / 2 waves of either kind for the whole measurement
    const int blocks = 256 * n * (vmix ? 1 : 4);
    hipFuncSetAttribute((const void*)k<OP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipMemset(arrivals, 0, CU_KEYS * 4);
    k<OP><<<blocks, 256, lds>>>(out, cyc, role, where, arrivals, 10, simds, vmix);
    hipDeviceSynchronize();
    hipMemset(arrivals, 0, CU_KEYS * 4);
    k<OP><<<blocks, 256, lds>>>(out, cyc, role, where, arrivals, ITERS, simds, vmix);
    if (hipDeviceSynchronize() != hipSuccess) { printf(" launch failed\n"); return; }
    std::vector<unsigned long long> h((size_t)blocks * 4);
    std::vector<int> r((size_t)blocks * 4);
    std::vector<uint32_t> w((size_t)blocks * 4);
    hipMemcpy(h.data(), cyc, h.size() * 8, hipMemcpyDeviceToHost);
    hipMemcpy(r.data(), role, r.size() * 4, hipMemcpyDeviceToHost);
    hipMemcpy(w.data(), where, w.size() * 4, hipMemcpyDeviceToHost);
    std::vector<unsigned long long> s, v;
    std::map<uint32_t, std::pair<int, int>> simd;  // (XCC, SE, SA, CU, SIMD) -> scalar waves, vector waves it held
    for (size_t i = 0; i < h.size(); i++) {
      if (r[i] == 1) { s.push_back(h[i]); simd[w[i]].first++; }
      if (r[i] == 2) { v.push_back(h[i]); simd[w[i]].second++; }
    }
    printf("  n=%d", n);
    if (!s.empty()) {
      // scalar waves per CU while one runs: simds SIMDs x n waves (x n / 2 beside vector waves)
      const double perCu = (double)simds * n / (vmix ? 2 : 1);
      printf(" %6.2f", median(s) / ((double)ITERS * REP * perCu));
    }
    if (!v.empty()) printf(" (valu %5.2f)", median(v) / ((double)ITERS * REP * n / 2));  // ticks per vector instruction per SIMD
    if (vmix == 1) {  // SIMDs that held exactly n / 2 waves of either kind, of the SIMDs that held any
      int both = 0;
      for (auto& e : simd) both += e.second.first == n / 2 && e.second.second == n / 2;
      printf(" [%d/%d]", both, (int)simd.size());
    }
  }
  printf("\n");
  hipFree(out); hipFree(cyc); hipFree(role); hipFree(where); hipFree(arrivals);
}

template <int OP>
void all(const char* name) {
  for (int simds : {1, 2, 4}) run<OP>(name, simds, 0);
  run<OP>(name, 4, 1);
}

int main() {
  printf("median s_memtime ticks per scalar instruction PER CU (per round trip for the last two), waves of `simds` SIMDs issuing,\n"
         "n waves per SIMD.  +valu: n / 2 of a SIMD's n waves run v_min_i32 instead (its ticks per vector instruction per SIMD;\n"
         "[SIMDs that held n / 2 waves of either kind / SIMDs that held a wave], from the hardware ids); valu alone: only those run\n");
  all<0>("s_add_i32");
  run<0>("v_min_i32", 4, 2);
  all<1>("s_and_b64");
  all<2>("s_cselect_b32");
  all<3>("s_bcnt1_i32_b64");
  all<4>("s_mov_b64 exec");
  all<5>("v_cmp..branch taken");
  all<6>("v_cmp..branch not taken");
  return 0;
}
