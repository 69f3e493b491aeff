// The distillation teacher's tail: raw four-channel pts3d head output -> points (optionally moved by a rigid transform per image) and
// confidences, in one streaming pass.  Declared in include/vicasplat_teacher.h (prefix vst_).
//
//   load     one thread per pixel, one 16-byte load (f32) or 8-byte load (f16) of x | y | z | c: a wave reads 1 KiB (512 B) in a row.
//   maths    f64 on the loaded values, rounded once: at d = 80 the f32 rounding of d alone moves expm1(d) by 40 units in the last place, and
//            two transcendentals in f64 per 32 bytes of traffic stay under the memory time.  expm1 becomes +inf where its f32 value does.
//   store    conf: lane l writes float l of the wave's 64.  pts: the wave's 64 pixels are 192 consecutive floats; in round r lane l
//            writes float 64 r + l, which it fetches from lane (64 r + l) / 3 by shuffles -- three fully coalesced 256-byte stores instead of
//            three stores of 4 bytes at a 12-byte stride.  No LDS is allocated.
//   ragged   every wave is whole (256 threads per block, no early return: the shuffles need all lanes); a lane past the last pixel loads
//            nothing and the stores are guarded by the float's index.
#include "common.h"

#include <cfloat>
#include <hip/hip_fp16.h>

#include "../../include/vicasplat_teacher.h"

namespace {

constexpr int kThreads = 256;

// a * b, skipping the product when a factor is zero: 0 * inf is 0 here (the header states it)
__device__ __forceinline__ double mul_skip(double a, double b) { return (a == 0.0 || b == 0.0) ? 0.0 : a * b; }

template <bool F16>
__global__ void __launch_bounds__(kThreads) points_conf_kernel(const void *__restrict__ raw, const float *__restrict__ transform,
                                                               int64_t count, int64_t plane, float *__restrict__ pts,
                                                               float *__restrict__ conf) {
    const int64_t pix = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = pix < count;
    float x = 0.f, y = 0.f, z = 0.f, c = 0.f;
    if (live) {
        if (F16) {
            const uint2 u = reinterpret_cast<const uint2 *>(raw)[pix];
            const float2 a = __half22float2(*reinterpret_cast<const __half2 *>(&u.x));
            const float2 b = __half22float2(*reinterpret_cast<const __half2 *>(&u.y));
            x = a.x; y = a.y; z = b.x; c = b.y;
        } else {
            const float4 v = reinterpret_cast<const float4 *>(raw)[pix];
            x = v.x; y = v.y; z = v.z; c = v.w;
        }
    }
    const double dx = x, dy = y, dz = z;
    const double d = sqrt(dx * dx + dy * dy + dz * dz);
    double e = expm1(d);
    if (e > (double)FLT_MAX) e = INFINITY;      // where expm1 overflows in f32, the reference's factor is +inf
    const double s = e / fmax(d, 1e-8);
    // a zero component stays an exact zero (0 * inf would be NaN)
    double px = x == 0.f ? 0.0 : dx * s, py = y == 0.f ? 0.0 : dy * s, pz = z == 0.f ? 0.0 : dz * s;
    if (transform && live) {
        // the image of the pixel: a 32-bit division where the pixel count allows (the 64-bit one is emulated: dozens of instructions)
        const int64_t img = count <= 0xffffffffLL ? (int64_t)((uint32_t)pix / (uint32_t)plane) : pix / plane;
        const float4 *T = reinterpret_cast<const float4 *>(transform + 12 * img);      // [3][4] rows of (R | t): 48 bytes per image
        const float4 r0 = T[0], r1 = T[1], r2 = T[2];
        const double qx = mul_skip(r0.x, px) + mul_skip(r0.y, py) + mul_skip(r0.z, pz) + (double)r0.w;
        const double qy = mul_skip(r1.x, px) + mul_skip(r1.y, py) + mul_skip(r1.z, pz) + (double)r1.w;
        const double qz = mul_skip(r2.x, px) + mul_skip(r2.y, py) + mul_skip(r2.z, pz) + (double)r2.w;
        px = qx; py = qy; pz = qz;
    }
    const float fx = (float)px, fy = (float)py, fz = (float)pz;
    if (live) conf[pix] = (float)(1.0 + exp((double)c));

    // the wave's 64 pixels -> 192 consecutive floats, 64 per round
    const int64_t wave_pix = pix - lane;
    float *out = pts + 3 * wave_pix;
    const int64_t left = 3 * (count - wave_pix);      // floats of this wave that exist (<= 0: none)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int f = 64 * r + lane, src = f / 3, comp = f - 3 * src;
        const float vx = __shfl(fx, src, 64), vy = __shfl(fy, src, 64), vz = __shfl(fz, src, 64);
        if (f < left) out[f] = comp == 0 ? vx : comp == 1 ? vy : vz;
    }
}

}  // namespace

extern "C" int vst_points_conf(const void *raw, int32_t raw_is_f16, const float *transform, int32_t n, int32_t H, int32_t W, float *pts,
                               float *conf, vs_stream_t stream_) {
    const char *who = "vst_points_conf";
    VS_CHECK(raw && pts && conf, "%s: null pointer (raw, pts and conf are required)", who);
    VS_CHECK(n > 0 && H > 0 && W > 0, "%s: n = %d, H = %d, W = %d must be positive", who, n, H, W);
    const int64_t plane = (int64_t)H * W, count = plane * n;
    const int64_t blocks = vs::cdiv64(count, kThreads);
    VS_CHECK(blocks <= INT32_MAX, "%s: %lld pixels are too many for one launch", who, (long long)count);
    VS_CHECK(((uintptr_t)raw & (raw_is_f16 ? 7 : 15)) == 0, "%s: raw is not %d-byte aligned", who, raw_is_f16 ? 8 : 16);
    VS_CHECK(((uintptr_t)pts & 3) == 0 && ((uintptr_t)conf & 3) == 0, "%s: pts or conf is not 4-byte aligned", who);
    VS_CHECK(!transform || ((uintptr_t)transform & 15) == 0, "%s: transform is not 16-byte aligned", who);
    const hipStream_t stream = (hipStream_t)stream_;
    if (raw_is_f16)
        hipLaunchKernelGGL(points_conf_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, raw, transform, count, plane, pts, conf);
    else
        hipLaunchKernelGGL(points_conf_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, raw, transform, count, plane, pts, conf);
    VS_HIP(hipGetLastError());
    return 0;
}
