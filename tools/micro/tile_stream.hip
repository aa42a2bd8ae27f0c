// Micro-benchmark: what the LAYOUT of an activation tensor costs the 1x1 convolutions of layer3 / layer4 in HBM efficiency.
// The LDS-DMA GEMM (csrc/conv.hip conv_dma_kernel) streams its pixel operand as k-tiles of 16 channels: one DMA instruction of a wave
// = 16 pixel rows x 64 bytes, the rows one whole NHWC pixel apart (K = 1024 channels: 4 KB).  Every access of the tile walk therefore
// opens another DRAM page; the epilogue writes 8 rows x 128 bytes per store instruction at the same 4 KB pitch.  This file runs the bare
// access patterns (no multiply) over 0.52 GB in three layouts:
//   0  row-major NHWC              [m][K * 4 B]                                 (what the tensors are today)
//   1  k-tile-major per 256 rows   [m / 256][k / 16][256 rows][64 B]            (a GEMM tile's k-tile is ONE contiguous 16 KB piece)
//   2  32 x 32 blocks              [m / 32][k / 32][32 rows][128 B]             (a wave's epilogue patch is one contiguous 4 KB piece)
// build + run on the GPU box:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/micro/tile_stream.hip -o /tmp/tile_stream && /tmp/tile_stream
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <algorithm>

#define LDSP(ptr_) ((__attribute__((address_space(3))) void*)(ptr_))

// (a function of its own: with the builtin called directly from the kernel template the HOST pass of hipcc drops the kernel's launch stub)
__device__ __forceinline__ void dma16(const __amdgpu_buffer_rsrc_t r, unsigned lds_addr, unsigned voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (__attribute__((address_space(3))) void*)(uintptr_t)lds_addr, 16, voff, 0, 0, 0);
}

// reader: one workgroup of NW waves per BM = 16 * NW row tile, NS stages in flight, k-tiles of 64 bytes per row
template <int MODE, int NW, int NS>
__global__ __launch_bounds__(NW * 64) void read_tiles(const unsigned char* A, int M, int nk, unsigned bytes, unsigned* sink, int shared) {
  constexpr int BM = NW * 16;
  __shared__ __attribute__((aligned(1024))) unsigned char st[NS][BM * 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = shared ? (int)blockIdx.x % shared : (int)blockIdx.x, drow = lane >> 2, pc = lane & 3;   // shared: every workgroup reads one of `shared` tiles (the WEIGHT operand: L2 hits)
  const int row = tile * BM + wave * 16 + drow;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(A), 0, bytes, 0x00020000);
  auto off = [&](int kt) -> unsigned {
    if (row >= M) return 0x80000000u;
    if (MODE == 0) return (unsigned)row * (unsigned)(nk * 64) + (unsigned)kt * 64u + (unsigned)pc * 16u;
    if (MODE == 1) return ((unsigned)(tile * nk + kt) * (unsigned)BM + (unsigned)(wave * 16 + drow)) * 64u + (unsigned)pc * 16u;
    return ((unsigned)(row / 32) * (unsigned)(nk / 2) + (unsigned)(kt / 2)) * 4096u + (unsigned)(row % 32) * 128u + (unsigned)(kt & 1) * 64u + (unsigned)pc * 16u;
  };
  const unsigned lds0 = (unsigned)(uintptr_t)LDSP(&st[0][0]) + (unsigned)wave * 1024u;
#pragma unroll
  for (int s = 0; s < NS - 1; s++) dma16(rs, lds0 + (unsigned)s * (BM * 64), off(s));
  unsigned acc = 0;
  for (int kt = 0; kt < nk; kt += NS) {
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const int nx = kt + s + NS - 1;
      dma16(rs, lds0 + (unsigned)((s + NS - 1) % NS) * (BM * 64), off(nx < nk ? nx : nk - 1));
      asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(NS - 1) : "memory");
      acc += *reinterpret_cast<const unsigned*>(&st[s][tid * 4 % (BM * 64)]);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (acc == 0x12345678u) sink[0] = acc;
}

// line-fetch reader (row-major tensor only): the same four 64-byte k-tile stages, but the two halves of a 128-byte line are requested together.
//   PAT 1: two 16-row x 64 B instructions back to back (k-tiles t, t + 1 into their two stages) at every even step, none at odd steps
//   PAT 2: two 8-row x 128 B instructions (whole lines, 1 KB contiguous in LDS; the four stages seen as two pair buffers of 128 B rows)
// A wave owns the same 16 rows either way.  At step t the stages of tiles t - 2 and t - 1 are free (second barrier of step t - 1).
template <int PAT, int NW>
__global__ __launch_bounds__(NW * 64) void read_lines(const unsigned char* A, int M, int nk, unsigned bytes, unsigned* sink) {
  constexpr int BM = NW * 16;
  __shared__ __attribute__((aligned(1024))) unsigned char st[4][BM * 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tile = (int)blockIdx.x;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(A), 0, bytes, 0x00020000);
  const unsigned pitch = (unsigned)nk * 64u, ldsb = (unsigned)(uintptr_t)LDSP(&st[0][0]);
  // PAT 1: lane = (row lane >> 2 of 16, 16-byte piece lane & 3 of a 64-byte half); PAT 2: lane = (row lane >> 3 of 8, piece lane & 7 of a line)
  const int r1 = tile * BM + wave * 16 + (lane >> 2), r2 = tile * BM + wave * 16 + (lane >> 3);
  const unsigned o1 = r1 < M ? (unsigned)r1 * pitch + (unsigned)(lane & 3) * 16u : 0x80000000u;
  const unsigned o2a = r2 < M ? (unsigned)r2 * pitch + (unsigned)(lane & 7) * 16u : 0x80000000u;
  const unsigned o2b = r2 + 8 < M ? o2a + 8u * pitch : 0x80000000u;
  auto pair = [&](int t) {                                  // k-tiles t (even) and t + 1
    const int tc = t < nk ? t : nk - 2;
    if (PAT == 1) {
      dma16(rs, ldsb + (unsigned)(t & 3) * (BM * 64) + (unsigned)wave * 1024u, o1 + (unsigned)tc * 64u);
      dma16(rs, ldsb + (unsigned)((t + 1) & 3) * (BM * 64) + (unsigned)wave * 1024u, o1 + (unsigned)tc * 64u + 64u);
    } else {
      const unsigned pb = ldsb + (unsigned)((t >> 1) & 1) * (BM * 128) + (unsigned)wave * 2048u;
      dma16(rs, pb, o2a + (unsigned)tc * 64u);
      dma16(rs, pb + 1024u, o2b + (unsigned)tc * 64u);
    }
  };
  pair(0);
  unsigned acc = 0;
  for (int kt = 0; kt < nk; kt += 4) {
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if ((s & 1) == 0) pair(kt + s + 2);
      // tile t landed: even t -- the second half of its pair and the pair just issued are younger (PAT 2: its pair is ONE group of two
      // instructions, the pair just issued is younger); odd t -- only the pair issued one step ago is younger
      if (PAT == 1 && (s & 1) == 0) asm volatile("s_waitcnt vmcnt(3)\n\ts_barrier" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2)\n\ts_barrier" ::: "memory");
      acc += *reinterpret_cast<const unsigned*>(&st[s][tid * 4 % (BM * 64)]);
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (acc == 0x12345678u) sink[0] = acc;
}

// writer: a wave owns 32 rows x 256 channels (8 patches of 32 x 32 channels = 32 rows x 128 B), four 16-byte stores per lane and patch
template <int MODE>
__global__ __launch_bounds__(256) void write_patches(unsigned char* O, int M, int ncb /* 32-channel blocks per row */, int cb0span) {
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int prow = lane >> 3, chunk = lane & 7;
  const int g = (int)blockIdx.x * 4 + wave;                 // wave id -> (row block of 32, group of cb0span channel blocks)
  const int groups = ncb / cb0span, rb = g / groups, cg = g % groups;
  if (rb * 32 >= M) return;
  const uint4 v = make_uint4(0x39993999u + lane, 0x39993999u, 0x39993999u, 0x39993999u);
  for (int j = 0; j < cb0span; j++) {
    const int cb = cg * cb0span + j;
#pragma unroll
    for (int it = 0; it < 4; it++) {
      const int r = rb * 32 + it * 8 + prow;
      size_t o;
      if (MODE == 0) o = (size_t)r * (size_t)(ncb * 128) + (size_t)cb * 128 + (size_t)chunk * 16;
      else o = ((size_t)rb * ncb + cb) * 4096 + (size_t)(it * 8 + prow) * 128 + (size_t)chunk * 16;
      *reinterpret_cast<uint4*>(O + o) = v;
    }
  }
}

template <typename F> static float best_of(F f, int reps = 7) {
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  float best = 1e9f;
  for (int r = 0; r < reps; r++) { hipEventRecord(e0); f(); hipEventRecord(e1); hipEventSynchronize(e1); float ms; hipEventElapsedTime(&ms, e0, e1); best = std::min(best, ms); }
  return best;
}

int main() {
  const int M = 128000, K = 1024, nk = K / 16;
  const size_t bytes = (size_t)M * K * 4;
  unsigned char* A; unsigned* sink; hipMalloc(&A, bytes); hipMalloc(&sink, 64); hipMemset(A, 1, bytes);
  const double gb = bytes / 1e9;
  printf("pixel operand of a 1x1 convolution, M = %d pixels x K = %d channels (%.2f GB), k-tiles of 16 channels, LDS-DMA, no multiply\n", M, K, gb);
#define RD(MODE, NW, NS, NAME) { const float ms = best_of([&] { hipLaunchKernelGGL((read_tiles<MODE, NW, NS>), dim3((M + NW * 16 - 1) / (NW * 16)), dim3(NW * 64), 0, 0, A, M, nk, (unsigned)bytes, sink, SHARED); }); \
    printf("  read  %-44s %d-row tiles, %d stages%s: %.3f ms  %.0f GB/s\n", NAME, NW * 16, NS, SHARED ? " (every workgroup the SAME tile: weight operand, L2 hits)" : "", ms, gb / ms * 1e3); }
  int SHARED = 0;
  RD(0, 16, 4, "row-major NHWC (4 KB pixel pitch)")
  RD(1, 16, 4, "k-tile-major per tile (16 KB pieces)")
  RD(2, 16, 4, "32 x 32 blocks (4 KB pieces)")
  RD(0, 8, 3, "row-major NHWC (4 KB pixel pitch)")
  RD(1, 8, 3, "k-tile-major per tile (8 KB pieces)")
  RD(2, 8, 3, "32 x 32 blocks (4 KB pieces)")
  // the two 64-byte halves of a 128-byte line: one k-tile apart (the RD(0, ...) rows above and (a) below), back to back (b), one instruction (c)
#define RL(PAT, NW, NAME) { const float ms = best_of([&] { hipLaunchKernelGGL((read_lines<PAT, NW>), dim3((M + NW * 16 - 1) / (NW * 16)), dim3(NW * 64), 0, 0, A, M, nk, (unsigned)bytes, sink); }); \
    printf("  read  %-44s %d-row tiles, 4 stages: %.3f ms  %.0f GB/s\n", NAME, NW * 16, ms, gb / ms * 1e3); }
  RD(0, 16, 4, "(a) 16 rows x 64 B, halves one k-tile apart")
  RL(1, 16, "(b) 16 rows x 64 B, halves back to back")
  RL(2, 16, "(c) 8 rows x 128 B per instruction")
  RD(0, 8, 4, "(a) 16 rows x 64 B, halves one k-tile apart")
  RL(1, 8, "(b) 16 rows x 64 B, halves back to back")
  RL(2, 8, "(c) 8 rows x 128 B per instruction")
  if (getenv("TILE_STREAM_LINES_ONLY")) return 0;          // (the one-counter pass over the three patterns)
  SHARED = 1;
  RD(0, 16, 4, "row-major [Cout][K] (4 KB row pitch)")
  RD(1, 16, 4, "k-tile-major (16 KB pieces)")
  SHARED = 4;
  RD(0, 16, 4, "row-major [Cout][K] (4 KB row pitch), 4 tiles")
  RD(1, 16, 4, "k-tile-major (16 KB pieces), 4 tiles")
  const int ncb = K / 32;
#define WR(MODE, SPAN, NAME) { const int waves = (M / 32) * (ncb / SPAN); const float ms = best_of([&] { hipLaunchKernelGGL((write_patches<MODE>), dim3((waves + 3) / 4), dim3(256), 0, 0, A, M, ncb, SPAN); }); \
    printf("  write %-44s a wave = 32 rows x %d channels: %.3f ms  %.0f GB/s\n", NAME, SPAN * 32, ms, gb / ms * 1e3); }
  WR(0, 2, "row-major NHWC (8 rows x 128 B per store)")
  WR(1, 2, "32 x 32 blocks (1 KB per store)")
  WR(0, 8, "row-major NHWC (8 rows x 128 B per store)")
  WR(1, 8, "32 x 32 blocks (1 KB per store)")
  return 0;
}
