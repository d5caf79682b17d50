// Growing contexts (npf_append_points): rows of a PT32 tensor [n_tasks][N][F] are placed into a PT32 tensor [n_tasks][M][F] behind the
// rows each task already holds.  The per-task offsets n_valid[task] -- and, optionally, how many of the N rows each task adds -- are
// data on the device: the host never reads them, so the launch sits in a captured graph and sees new counts at every replay.
//
// Two launches in stream order.  append_rows_kernel only READS the counts and writes rows of dst; append_counts_kernel then advances
// the counts.  No workgroup can therefore see a count another has already advanced, and no atomics are needed.
#include "npf_common.hpp"

namespace npf {

struct AppendArgs {
  npf_append_pair_t pair[NPF_APPEND_MAX_PAIRS];
};

// grid = (source tiles x chunks of 32 feature quads, n_tasks, n_pairs); 256 threads = 8 feature quads x 32 rows, every thread moves up to
// four 16-byte (row, 4 features) units: 32 consecutive lanes read 512 consecutive bytes of a source tile and write at most two
// consecutive runs of the destination (the destination rows of one source tile straddle at most one tile boundary).
__global__ __launch_bounds__(256) void append_rows_kernel(AppendArgs a, const int32_t* __restrict__ n_valid,
                                                          const int32_t* __restrict__ n_new, int N, int M) {
  const npf_append_pair_t pr = a.pair[blockIdx.z];
  const int F4 = pr.F / 4;
  const int chunks = (F4 + 31) / 32;
  const int tile = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const size_t task = blockIdx.y;
  const int p = threadIdx.x & 31, q = threadIdx.x >> 5;
  // rows the task holds / adds, clamped to what the tensors hold
  const int have = clamp_count(n_valid, task, M);
  const int add = n_new ? clamp_count(n_new, task, N) : N;
  const int j = tile * 32 + p;       // source row
  const int row = have + j;          // destination row
  if (chunk >= chunks || j >= add || row >= M) return;  // (rows at or beyond the capacity are dropped)
  const int tilesN = (N + 31) / 32, tilesM = (M + 31) / 32;
  const float* s = pr.src + (task * tilesN + tile) * (size_t)(pr.F * 32);
  float* d = pr.dst + (task * tilesM + (row >> 5)) * (size_t)(pr.F * 32);
  const int f0 = chunk * 32 + q;
  f32x4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (f0 + 8 * k < F4) v[k] = *(const f32x4*)(s + pt_off(f0 + 8 * k, p));
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (f0 + 8 * k < F4) *(f32x4*)(d + pt_off(f0 + 8 * k, row & 31)) = v[k];
}

__global__ void append_counts_kernel(int32_t* __restrict__ n_valid, const int32_t* __restrict__ n_new, int n_tasks, int N, int M) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_tasks) return;
  const int have = clamp_count(n_valid, b, M);
  const int add = n_new ? clamp_count(n_new, b, N) : N;
  n_valid[b] = have + add < M ? have + add : M;
}

}  // namespace npf

extern "C" int npf_append_points(const npf_append_pair_t* pairs, int32_t n_pairs, int32_t* n_valid, const int32_t* n_new,
                                 int32_t n_tasks, int32_t n_rows, int32_t capacity, void* stream) {
  if (!pairs || n_pairs < 1 || n_pairs > NPF_APPEND_MAX_PAIRS || !n_valid || n_tasks < 0 || n_tasks > 65535 || n_rows < 0 ||
      capacity <= 0)
    return NPF_EINVAL;
  npf::AppendArgs a = {};
  int maxF = 0;
  for (int i = 0; i < n_pairs; ++i) {
    const npf_append_pair_t& p = pairs[i];
    if (!p.src || !p.dst || p.F <= 0 || (p.F & 31) || ((((uintptr_t)p.src) | ((uintptr_t)p.dst)) & 15)) return NPF_EINVAL;
    a.pair[i] = p;
    if (p.F > maxF) maxF = p.F;
  }
  if (n_tasks == 0 || n_rows == 0) return NPF_OK;
  const int tilesN = (n_rows + 31) / 32, chunks = (maxF / 4 + 31) / 32;
  hipLaunchKernelGGL(npf::append_rows_kernel, dim3((unsigned)(tilesN * chunks), (unsigned)n_tasks, (unsigned)n_pairs), dim3(256), 0,
                     (hipStream_t)stream, a, (const int32_t*)n_valid, n_new, n_rows, capacity);
  NPF_CHECK_LAUNCH();
  hipLaunchKernelGGL(npf::append_counts_kernel, dim3((unsigned)((n_tasks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_valid,
                     n_new, n_tasks, n_rows, capacity);
  NPF_CHECK_LAUNCH();
  return NPF_OK;
}
