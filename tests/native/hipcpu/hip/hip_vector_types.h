// Vector types of the HIP stand-in (see hip_runtime.h in this directory): size and alignment of the device's.
#pragma once

#include <stdint.h>

#define HIPCPU_VEC2(name, T, A) \
    struct alignas(A) name { T x, y; }; \
    static inline name make_##name(T x, T y) { return name{x, y}; }
#define HIPCPU_VEC4(name, T, A) \
    struct alignas(A) name { T x, y, z, w; }; \
    static inline name make_##name(T x, T y, T z, T w) { return name{x, y, z, w}; }

HIPCPU_VEC2(int2, int, 8)
HIPCPU_VEC2(uint2, unsigned int, 8)
HIPCPU_VEC4(int4, int, 16)
HIPCPU_VEC4(uint4, unsigned int, 16)
HIPCPU_VEC2(longlong2, long long, 16)
HIPCPU_VEC2(ulonglong2, unsigned long long, 16)

struct uint3 { unsigned int x, y, z; };
struct dim3 {
    unsigned int x, y, z;
    constexpr dim3(unsigned int x_ = 1, unsigned int y_ = 1, unsigned int z_ = 1) : x(x_), y(y_), z(z_) {}
};
