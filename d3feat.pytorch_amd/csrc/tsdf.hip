// The bounds of the depth frames of a batch of dense TSDF volumes (include/d3feat_hip.h: d3f_tsdf_bounds; the rule is
// csrc/tsdf.hpp).  What follows them is elsewhere: the integration, d3f_tsdf_integrate, in csrc/tsdf_integrate.hip, the
// extraction of the zero crossings, d3f_tsdf_extract, in csrc/tsdf_extract.hip.
//   bounds     one workgroup per 2048 pixels of one frame: the frame and its volume are workgroup-uniform, a wave folds
//              its keys by shuffles and one lane issues six integer min / max atomics on the ordered keys (exact, so
//              the order of arrival cannot matter).
// The host twin runs the same tsdf.hpp text on the CPU and makes no GPU call.
#include "tsdf_batch.hpp"   // the frames, the argument checks

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

}  // extern "C"
