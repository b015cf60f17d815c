// hrt_launch_dir.h -- the launch direction of a global path index on the device, shared by
// hrt_launch_dirs_kernel (csrc/hrt_kernels.hip) and the array channel (csrc/hrt_array_channel.hip, where it is
// the departure direction of a scatter record).  HIP device code only.
//
// The reference evaluates (src/compute_paths.c:444-451)
//   k = p + .5f; phi = (float)acos(1.f - 2.f*k/N); theta = pi_f*(1.f + sqrtf(5.f))*k   (float)
//   d = ((float)(cos(theta)*sin(phi)), (float)(sin(theta)*sin(phi)), (float)cos(phi))   (double libm)
// The float steps are exact IEEE operations; the double ones use the device library (see
// hrt_launch_dirs_kernel for how its last bits are kept out of the rounded result there).
#ifndef HRT_LAUNCH_DIR_H
#define HRT_LAUNCH_DIR_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// global path of local ray i of shard `rank` of `count` (hrt_shard_global_path)
__device__ __forceinline__ uint64_t hrt_shard_path(uint64_t i, uint32_t chunk, uint32_t count, uint32_t rank)
{
    return ((i / chunk) * count + rank) * chunk + i % chunk;
}

// the double values before their rounding to float, and the floats (d = (fx, fy, fz))
struct hrt_launch_dir_t {
    double ph_d, x, y, z;
    float phi, fx, fy, fz;
};

__device__ __forceinline__ hrt_launch_dir_t hrt_launch_dir(uint64_t p, uint64_t num_paths)
{
#pragma clang fp contract(off)
    const float pi_f = 3.14159265358979323846f;   // src/compute_paths.c:18 (float)
    hrt_launch_dir_t r;
    const float k = (float)p + .5f;
    const float arg = 1.f - 2.f * k / (float)num_paths;
    r.ph_d = acos((double)arg);
    r.phi = (float)r.ph_d;
    const float theta = pi_f * (1.f + sqrtf(5.f)) * k;
    const double sp = sin((double)r.phi);
    r.x = cos((double)theta) * sp;
    r.y = sin((double)theta) * sp;
    r.z = cos((double)r.phi);
    r.fx = (float)r.x;
    r.fy = (float)r.y;
    r.fz = (float)r.z;
    return r;
}

#endif  // HRT_LAUNCH_DIR_H
