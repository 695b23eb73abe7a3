// A CPU stand-in for the part of the HIP runtime and of the gfx950 device language that sgfhe.jl_amd/csrc uses.
// Test infrastructure only: with this directory first on the include path, engine.hip and its kernel headers compile
// unchanged as host C++ (clang++ -x c++), so that AddressSanitizer, UBSan and gdb see every kernel and every buffer the
// host code sizes.  Nothing under sgfhe.jl_amd/ or bench.py includes it.  The other half is hipcpu.cpp.
//
// Memory.  hipMalloc is malloc of exactly the bytes asked (a sanitizer's red zone sits at the true end), filled with
// the byte HIPCPU_FILL names (default 0): two runs under two bytes differ wherever an output depends on device memory
// that nothing wrote.  hipHostMalloc is the same; the copies and memsets are memcpy and memset.
//
// Streams and events.  Every operation runs to completion at the call (one legal serialisation of stream order).
// Events do nothing, hipEventElapsedTime gives 0, hipGetDeviceCount gives 1.  hipFuncSetAttribute records the
// dynamic-LDS limit of a kernel (64 KiB without it), and a launch that asks for more fails as on the device.
//
// A launch.  The blocks run one after another (static __shared__ is `static`); the threads of a block are OS threads
// of a pool sized by the block dimension (1024 at most, never by the machine's CPU count).  threadIdx, blockIdx,
// blockDim and gridDim are thread_local.  __syncthreads is a barrier over the block's threads that have not returned
// (a waiting thread gives its core away a few times before it sleeps: a block has more threads than the machine cores).
// The wavefront fence (the exchange inside one wave in ntt.h) is a barrier over the 64 lanes of the calling wave: the
// device code relies on lockstep there, and a barrier is the conservative reading.  __shfl_xor exchanges through a
// slot per lane between two wave barriers.  __builtin_amdgcn_readfirstlane returns the value of the first lane still
// running and aborts when the calling lane's differs (the code claims uniformity wherever it uses it).  A lane that
// has returned takes no part: a shuffle from it gives the caller's own value.  Atomics are the __atomic builtins.
// Dynamic LDS is a fresh 16-byte aligned heap block of exactly the launch's byte count (the sanitizer's red zone
// begins at that byte, not at the next multiple of 16), refilled with the fill byte before each block and freed after
// the launch: an LDS overrun is a heap-buffer-overflow.
// A kernel whose first launch reached no barrier, fence, shuffle or readfirstlane runs its later launches as a plain
// loop over blocks and threads; reaching one of them in that form aborts ("... in a kernel that ran as a plain loop").
// The decision is per launch site and taken once: a kernel that can leave every block before its first barrier in one
// launch and reach it in another (k_circ_split, when no input is read) would be judged by whichever came first, so
// hipcpu.cpp lists such kernels in ALWAYS_THREADED.
//
// Buffer resources.  Loads and stores keep the range check (a load gives 0, a store is dropped), here over the whole
// byte offset voffset + soffset (the hardware leaves soffset out: this is the stricter reading).  Every out-of-range
// access is counted per kernel, and aborts the program with the kernel's name unless hipcpu.cpp's allow-list names
// the kernel with its reason.
//
// Not modelled: timing, overlap of streams, wave scheduling beyond the three primitives above, the cache policy bits.
// Every launch is counted by kernel name; HIPCPU_LAUNCH_LOG names a file that receives the counts at exit.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <tuple>
#include <type_traits>
#include <utility>

#include "hip_vector_types.h"

#define SGFHE_HOST_KERNELS 1

#define __global__ static
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(...)

typedef enum hipError_t {
    hipSuccess = 0,
    hipErrorInvalidValue = 1,
    hipErrorOutOfMemory = 2,
    hipErrorInvalidConfiguration = 9
} hipError_t;
typedef enum hipMemcpyKind {
    hipMemcpyHostToHost = 0,
    hipMemcpyHostToDevice = 1,
    hipMemcpyDeviceToHost = 2,
    hipMemcpyDeviceToDevice = 3
} hipMemcpyKind;
typedef enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize = 8 } hipFuncAttribute;
typedef struct ihipStream_t *hipStream_t;
typedef struct ihipEvent_t *hipEvent_t;
#define hipHostMallocDefault 0u
#define hipStreamNonBlocking 1u
#define hipEventDisableTiming 2u

hipError_t hipGetLastError();
const char *hipGetErrorString(hipError_t e);
hipError_t hipGetDeviceCount(int *n);
hipError_t hipSetDevice(int d);
hipError_t hipMalloc(void **p, size_t bytes);
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags);
hipError_t hipFree(void *p);
hipError_t hipHostFree(void *p);
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind);
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t s);
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                            hipMemcpyKind kind, hipStream_t s);
hipError_t hipMemset(void *p, int v, size_t bytes);
hipError_t hipMemsetAsync(void *p, int v, size_t bytes, hipStream_t s);
hipError_t hipStreamCreate(hipStream_t *s);
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags);
hipError_t hipStreamDestroy(hipStream_t s);
hipError_t hipStreamSynchronize(hipStream_t s);
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned flags);
hipError_t hipEventCreate(hipEvent_t *e);
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags);
hipError_t hipEventDestroy(hipEvent_t e);
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s);
hipError_t hipEventSynchronize(hipEvent_t e);
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b);
hipError_t hipFuncSetAttribute(const void *func, hipFuncAttribute attr, int value);
template <class T>
hipError_t hipMalloc(T **p, size_t bytes) { return hipMalloc(reinterpret_cast<void **>(p), bytes); }
template <class T>
hipError_t hipHostMalloc(T **p, size_t bytes, unsigned flags) { return hipHostMalloc(reinterpret_cast<void **>(p), bytes, flags); }

extern thread_local uint3 threadIdx, blockIdx;
extern thread_local dim3 blockDim, gridDim;

namespace hipcpu {

void *dynamic_lds();
void syncthreads();
void wave_barrier();
uint64_t shfl_xor64(uint64_t v, int lane_mask);
uint32_t readfirstlane(uint32_t v);
void buffer_out_of_range();
void launch_blocks(const char *text, const void *func, dim3 grid, dim3 block, size_t lds, void (*thread_fn)(void *),
                   void *ctx);

template <class... P, class... A>
void launch(const char *text, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t, A &&...a) {
    struct Ctx {
        void (*kernel)(P...);
        std::tuple<std::decay_t<P>...> args;
    } ctx{kernel, std::tuple<std::decay_t<P>...>{std::forward<A>(a)...}};
    launch_blocks(text, reinterpret_cast<const void *>(kernel), grid, block, lds,
                  [](void *p) {
                      Ctx *c = static_cast<Ctx *>(p);
                      std::apply(c->kernel, c->args);
                  },
                  &ctx);
}

// the buffer resource of kernels.h: base and byte count (stride 0, raw addressing)
struct Rsrc {
    char *base;
    uint32_t bytes;
};
inline Rsrc make_rsrc(void *base, short, int bytes, int) { return Rsrc{static_cast<char *>(base), (uint32_t)bytes}; }
template <class T>
inline T buf_load(Rsrc r, int voff, int soff) {
    const uint64_t off = (uint64_t)(uint32_t)voff + (uint32_t)soff;
    T v;
    if (off + sizeof(T) > r.bytes) {
        buffer_out_of_range();
        memset(&v, 0, sizeof v);
    } else {
        memcpy(&v, r.base + off, sizeof v);
    }
    return v;
}
template <class T>
inline void buf_store(T v, Rsrc r, int voff, int soff) {
    const uint64_t off = (uint64_t)(uint32_t)voff + (uint32_t)soff;
    if (off + sizeof(T) > r.bytes) buffer_out_of_range();
    else memcpy(r.base + off, &v, sizeof v);
}
typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));

}  // namespace hipcpu

// (kernel, grid, block, lds bytes, stream, arguments...): a kernel name with commas arrives in parentheses
#define hipLaunchKernelGGL(kernel, ...) hipcpu::launch(#kernel, kernel, __VA_ARGS__)

#define __syncthreads() hipcpu::syncthreads()
#define __builtin_amdgcn_fence(order, scope) hipcpu::wave_barrier()
#define __builtin_amdgcn_sched_barrier(mask) ((void)0)
#define __builtin_amdgcn_readfirstlane(x) hipcpu::readfirstlane(x)
#define __amdgpu_buffer_rsrc_t hipcpu::Rsrc
#define __builtin_amdgcn_make_buffer_rsrc hipcpu::make_rsrc
#define __builtin_amdgcn_raw_buffer_load_b8(r, v, s, aux) hipcpu::buf_load<uint8_t>(r, v, s)
#define __builtin_amdgcn_raw_buffer_load_b16(r, v, s, aux) hipcpu::buf_load<uint16_t>(r, v, s)
#define __builtin_amdgcn_raw_buffer_load_b32(r, v, s, aux) hipcpu::buf_load<uint32_t>(r, v, s)
#define __builtin_amdgcn_raw_buffer_load_b128(r, v, s, aux) hipcpu::buf_load<hipcpu::v4u32>(r, v, s)
#define __builtin_amdgcn_raw_buffer_store_b32(val, r, v, s, aux) hipcpu::buf_store<uint32_t>(val, r, v, s)

static inline unsigned int __umulhi(unsigned int a, unsigned int b) { return (unsigned int)(((uint64_t)a * b) >> 32); }
static inline unsigned long long __umul64hi(unsigned long long a, unsigned long long b) {
    return (unsigned long long)(((unsigned __int128)a * b) >> 64);
}
static inline unsigned int __brev(unsigned int x) { return __builtin_bitreverse32(x); }
template <class T>
static inline T __shfl_xor(T v, int lane_mask, int width = 64) {
    static_assert(sizeof(T) <= 8 && std::is_trivially_copyable<T>::value, "a word of at most 64 bits");
    (void)width;
    uint64_t w = 0;
    memcpy(&w, &v, sizeof v);
    w = hipcpu::shfl_xor64(w, lane_mask);
    memcpy(&v, &w, sizeof v);
    return v;
}
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) {
    return __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
}
static inline unsigned int atomicAdd(unsigned int *p, unsigned int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
static inline unsigned long long atomicMax(unsigned long long *p, unsigned long long v) {
    unsigned long long old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static inline unsigned int atomicMax(unsigned int *p, unsigned int v) {
    unsigned int old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
static inline unsigned int atomicOr(unsigned int *p, unsigned int v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
