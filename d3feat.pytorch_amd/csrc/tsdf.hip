// The bounds of the depth frames of a batch of dense TSDF volumes and the extraction of the volumes' zero crossings
// (include/d3feat_hip.h: d3f_tsdf_bounds, d3f_tsdf_extract; the rule is csrc/tsdf.hpp).  The integration between the
// two, d3f_tsdf_integrate, is csrc/tsdf_integrate.hip.
//   bounds     one workgroup per 2048 pixels of one frame: the frame and its volume are workgroup-uniform, a wave folds
//              its keys by shuffles and one lane issues six integer min / max atomics on the ordered keys (exact, so
//              the order of arrival cannot matter).
//   extract    count per block of 256 voxels -> exclusive scan of the block counts in two levels (groups of 1024
//              counts, coalesced, then the group totals) -> emit, which recomputes the crossings and writes at
//              group offset + block offset + in-block rank (ballots + a prefix over the four waves).  No atomic
//              decides a position.
// The host twins run the same tsdf.hpp text on the CPU and make no GPU call.
#include "tsdf_batch.hpp"   // the batch, the frames, locate(), the argument checks, the two-level scan

namespace {

using namespace d3f::tsdf;

constexpr int kBoundsPixels = 8;          // pixels per thread of the bounds kernel

// ---------------------------------------------------------------------------------------------------------- bounds
__global__ void __launch_bounds__(kThreads) bounds_init_kernel(uint32_t* keys, int V) {
  const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (i < 6 * V) keys[i] = (i % 6) < 3 ? kKeyPosInf : kKeyNegInf;
}

__global__ void __launch_bounds__(kThreads) bounds_decode_kernel(uint32_t* keys, int V) {
  const int i = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (i < 6 * V) keys[i] = float_bits(order_value(keys[i]));
}

template <typename DepthT>
__global__ void __launch_bounds__(kThreads) bounds_kernel(const DepthT* __restrict__ images, int F, int H, int W,
                                                          const int32_t* __restrict__ frame_start, int V,
                                                          const float* __restrict__ K, const float* __restrict__ C,
                                                          float depth_scale, float depth_max, uint32_t* keys) {
  const int f = (int)blockIdx.y;
  if (f < frame_start[0] || f >= frame_start[V]) return;          // a frame no volume owns
  const int v = owner(frame_start, V, (int32_t)f);
  const int pixels = H * W;
  const DepthT* image = images + (size_t)pixels * (size_t)f;
  uint32_t lo[3] = {kKeyPosInf, kKeyPosInf, kKeyPosInf}, hi[3] = {kKeyNegInf, kKeyNegInf, kKeyNegInf};
  bool any = false;
  for (int k = 0; k < kBoundsPixels; ++k) {
    const int p = ((int)blockIdx.x * kBoundsPixels + k) * kThreads + (int)threadIdx.x;
    if (p >= pixels) break;
    float q[3];
    if (!back_project(image, W, p % W, p / W, K + 4 * (size_t)f, C + 12 * (size_t)f, depth_scale, depth_max, q))
      continue;
    any = true;
    for (int r = 0; r < 3; ++r) {
      const uint32_t key = order_key(q[r]);
      lo[r] = min(lo[r], key);
      hi[r] = max(hi[r], key);
    }
  }
  if (!__any(any)) return;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      lo[r] = min(lo[r], (uint32_t)__shfl_xor((int)lo[r], o, 64));
      hi[r] = max(hi[r], (uint32_t)__shfl_xor((int)hi[r], o, 64));
    }
  if (d3f::lane_id() == 0)
    for (int r = 0; r < 3; ++r) {
      atomicMin(keys + 6 * (size_t)v + r, lo[r]);
      atomicMax(keys + 6 * (size_t)v + 3 + r, hi[r]);
    }
}

template <typename DepthT>
void bounds_host(const DepthT* images, int F, int H, int W, const int32_t* frame_start, int V, const float* K,
                 const float* C, float depth_scale, float depth_max, float* bounds) {
  for (int v = 0; v < V; ++v) {
    uint32_t lo[3] = {kKeyPosInf, kKeyPosInf, kKeyPosInf}, hi[3] = {kKeyNegInf, kKeyNegInf, kKeyNegInf};
    const int f0 = frame_start[v] < 0 ? 0 : frame_start[v], f1 = frame_start[v + 1] > F ? F : frame_start[v + 1];
    for (int f = f0; f < f1; ++f) {
      const DepthT* image = images + (size_t)H * (size_t)W * (size_t)f;
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
          float q[3];
          if (!back_project(image, W, x, y, K + 4 * (size_t)f, C + 12 * (size_t)f, depth_scale, depth_max, q)) continue;
          for (int r = 0; r < 3; ++r) {
            const uint32_t key = order_key(q[r]);
            lo[r] = key < lo[r] ? key : lo[r];
            hi[r] = key > hi[r] ? key : hi[r];
          }
        }
    }
    for (int r = 0; r < 3; ++r) {
      bounds[6 * (size_t)v + r] = order_value(lo[r]);
      bounds[6 * (size_t)v + 3 + r] = order_value(hi[r]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------- extract
struct ExtractWs : BlockScan {
  size_t bytes;
  ExtractWs(void* ws, int64_t blocks) {
    d3f::Carver c(ws);
    carve(c, blocks);
    bytes = d3f::align_up(c.off, 256);
  }
};

// the crossings of global voxel g of volume v (bit a: axis a emits); a neighbour beyond the volume's own voxel range
// (vol_start and dims that disagree) is never read
__host__ __device__ inline int voxel_mask(const Volumes& b, const float* D, const float* w, float min_weight, int v,
                                          int64_t g, int64_t& local, int& ix, int& iy, int& iz, int& nx, int& ny) {
  int nz;
  const int64_t base = b.vol_start[v];
  local = g - base;
  locate(b, v, local, ix, iy, iz, nx, ny, nz);
  return crossings(D + base, w + base, local, b.vol_start[v + 1] - base, ix, iy, iz, nx, ny, nz, min_weight);
}

__global__ void __launch_bounds__(kThreads) extract_count_kernel(Volumes b, const float* __restrict__ D,
                                                                 const float* __restrict__ w, float min_weight,
                                                                 int32_t* __restrict__ block_count) {
  __shared__ int wave_total[kThreads / D3F_WAVE];
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int n = 0;
  if (g < b.total) {
    int64_t local;
    int ix, iy, iz, nx, ny;
    n = popcount3(voxel_mask(b, D, w, min_weight, owner(b.vol_start, b.V, g), g, local, ix, iy, iz, nx, ny));
  }
  n = d3f::wave_sum_i(n);
  if (d3f::lane_id() == 0) wave_total[threadIdx.x / D3F_WAVE] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
    for (int k = 0; k < kThreads / D3F_WAVE; ++k) s += wave_total[k];
    block_count[blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(kThreads) extract_emit_kernel(Volumes b, const float* __restrict__ D,
                                                                const float* __restrict__ w, float min_weight,
                                                                const int64_t* __restrict__ block_offset,
                                                                const int64_t* __restrict__ group_offset,
                                                                int64_t capacity, float* __restrict__ points,
                                                                int64_t* __restrict__ point_start, int32_t* status) {
  __shared__ int wave_total[kThreads / D3F_WAVE];
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = g < b.total;
  int mask = 0, v = 0, ix = 0, iy = 0, iz = 0, nx = 1, ny = 1;
  int64_t local = 0;
  if (live) {
    v = owner(b.vol_start, b.V, g);
    mask = voxel_mask(b, D, w, min_weight, v, g, local, ix, iy, iz, nx, ny);
  }
  const int lane = d3f::lane_id(), wave = (int)threadIdx.x / D3F_WAVE;
  const unsigned long long below = (1ull << lane) - 1ull;
  int before = 0, total = 0;   // points of the lower lanes of this wave; of the whole wave
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const unsigned long long m = __ballot((mask >> a) & 1);
    before += __popcll(m & below);
    total += __popcll(m);
  }
  if (lane == 0) wave_total[wave] = total;
  __syncthreads();
  for (int k = 0; k < wave; ++k) before += wave_total[k];
  if (!live) return;
  int64_t pos = group_offset[blockIdx.x / kScanThreads] + block_offset[blockIdx.x] + before;
  if (local == 0) point_start[v] = pos;         // the first voxel of a volume: where the volume's points begin
  bool overflow = false;
  for (int a = 0; a < 3; ++a) {
    if (!((mask >> a) & 1)) continue;
    if (pos < capacity)
      crossing_point(D + b.vol_start[v], local, ix, iy, iz, nx, ny, a, b.origin + 3 * v, b.voxel[v], points + 3 * pos);
    else
      overflow = true;
    ++pos;
  }
  if (overflow) atomicOr(status, D3F_TSDF_ST_OVERFLOW);
}

// -------------------------------------------------------------------------------------------------- argument checks
int run_extract_count(const Volumes& b, const float* D, const float* w, float min_weight, int64_t* point_start,
                      const ExtractWs& x, int64_t blocks, hipStream_t stream) {
  extract_count_kernel<<<(unsigned)blocks, kThreads, 0, stream>>>(b, D, w, min_weight, x.block_count);
  D3F_LAUNCH_CHECK();
  return run_block_scan(x, blocks, point_start + b.V, stream);
}

}  // namespace

extern "C" {

int d3f_tsdf_bounds(const void* depth, int depth_is_f32, int F, int H, int W, const int32_t* frame_start, int V,
                    const float* intrinsics, const float* camera_to_volume, float depth_scale, float depth_max,
                    float* bounds, void* stream) {
  if (!batch_ok(V, 0) || !bounds ||
      !frames_ok(depth, F, H, W, frame_start, intrinsics, camera_to_volume, depth_scale, depth_max) || F > 65535)
    return D3F_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  uint32_t* keys = (uint32_t*)bounds;
  bounds_init_kernel<<<d3f::cdiv(6 * V, kThreads), kThreads, 0, s>>>(keys, V);
  D3F_LAUNCH_CHECK();
  if (F > 0) {
    const dim3 grid((unsigned)d3f::cdiv((int64_t)H * W, kThreads * kBoundsPixels), (unsigned)F);
    if (depth_is_f32)
      bounds_kernel<float><<<grid, kThreads, 0, s>>>((const float*)depth, F, H, W, frame_start, V, intrinsics,
                                                     camera_to_volume, depth_scale, depth_max, keys);
    else
      bounds_kernel<uint16_t><<<grid, kThreads, 0, s>>>((const uint16_t*)depth, F, H, W, frame_start, V, intrinsics,
                                                        camera_to_volume, depth_scale, depth_max, keys);
    D3F_LAUNCH_CHECK();
  }
  bounds_decode_kernel<<<d3f::cdiv(6 * V, kThreads), kThreads, 0, s>>>(keys, V);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_bounds_host(const void* depth, int depth_is_f32, int F, int H, int W, const int32_t* frame_start, int V,
                         const float* intrinsics, const float* camera_to_volume, float depth_scale, float depth_max,
                         float* bounds, void* stream) {
  (void)stream;
  if (!batch_ok(V, 0) || !bounds ||
      !frames_ok(depth, F, H, W, frame_start, intrinsics, camera_to_volume, depth_scale, depth_max) || F > 65535)
    return D3F_EINVAL;
  if (depth_is_f32)
    bounds_host((const float*)depth, F, H, W, frame_start, V, intrinsics, camera_to_volume, depth_scale, depth_max,
                bounds);
  else
    bounds_host((const uint16_t*)depth, F, H, W, frame_start, V, intrinsics, camera_to_volume, depth_scale, depth_max,
                bounds);
  return D3F_OK;
}

size_t d3f_tsdf_extract_ws_bytes(int64_t total_voxels) {
  if (total_voxels < 0) return 0;
  return ExtractWs(nullptr, voxel_blocks(total_voxels)).bytes + 256;
}

int d3f_tsdf_extract_count(const float* D, const float* w, const int64_t* vol_start, const int32_t* dims, int V,
                           int64_t total_voxels, float min_weight, int64_t* point_start, void* ws, size_t ws_bytes,
                           void* stream) {
  const int64_t blocks = voxel_blocks(total_voxels);
  if (!batch_ok(V, total_voxels) || total_voxels == 0 || blocks > 0x7fffffff || !D || !w || !vol_start || !dims ||
      !point_start || !ws)
    return D3F_EINVAL;
  const ExtractWs x(ws, blocks);
  if (ws_bytes < x.bytes) return D3F_EWORKSPACE;
  const Volumes b = {vol_start, nullptr, dims, nullptr, V, total_voxels};
  return run_extract_count(b, D, w, min_weight, point_start, x, blocks, (hipStream_t)stream);
}

int d3f_tsdf_extract(const float* D, const float* w, const int64_t* vol_start, const float* origin,
                     const int32_t* dims, const float* voxel, int V, int64_t total_voxels, float min_weight,
                     int counted, int64_t capacity, float* points, int64_t* point_start, int32_t* status, void* ws,
                     size_t ws_bytes, void* stream) {
  const int64_t blocks = voxel_blocks(total_voxels);
  if (!batch_ok(V, total_voxels) || total_voxels == 0 || blocks > 0x7fffffff || !D || !w || !vol_start || !origin ||
      !dims || !voxel || !point_start || !status || !ws || capacity < 0 || (capacity > 0 && !points))
    return D3F_EINVAL;
  const ExtractWs x(ws, blocks);
  if (ws_bytes < x.bytes) return D3F_EWORKSPACE;
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  if (!counted) {
    const int rc = run_extract_count(b, D, w, min_weight, point_start, x, blocks, (hipStream_t)stream);
    if (rc != D3F_OK) return rc;
  }
  extract_emit_kernel<<<(unsigned)blocks, kThreads, 0, (hipStream_t)stream>>>(
      b, D, w, min_weight, x.block_offset, x.group_offset, capacity, points, point_start, status);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_extract_host(const float* D, const float* w, const int64_t* vol_start, const float* origin,
                          const int32_t* dims, const float* voxel, int V, int64_t total_voxels, float min_weight,
                          int64_t capacity, float* points, int64_t* point_start, int32_t* status) {
  if (!batch_ok(V, total_voxels) || total_voxels == 0 || !D || !w || !vol_start || !origin || !dims || !voxel ||
      !point_start || !status || capacity < 0 || (capacity > 0 && !points) ||
      !host_layout_ok(vol_start, dims, V, total_voxels))
    return D3F_EINVAL;
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  int64_t pos = 0;
  for (int v = 0; v < V; ++v) {
    point_start[v] = pos;
    for (int64_t g = vol_start[v]; g < vol_start[v + 1]; ++g) {
      int64_t local;
      int ix, iy, iz, nx, ny;
      const int mask = voxel_mask(b, D, w, min_weight, v, g, local, ix, iy, iz, nx, ny);
      for (int a = 0; a < 3; ++a) {
        if (!((mask >> a) & 1)) continue;
        if (pos < capacity)
          crossing_point(D + vol_start[v], local, ix, iy, iz, nx, ny, a, origin + 3 * v, voxel[v], points + 3 * pos);
        else
          *status |= D3F_TSDF_ST_OVERFLOW;
        ++pos;
      }
    }
  }
  point_start[V] = pos;
  return D3F_OK;
}

}  // extern "C"
