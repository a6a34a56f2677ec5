// TEST HARNESS: <hip/hip_runtime.h> for the device-code tier (tests/c/README.md, "Device code on the CPU").  A host compiler that is
// given this directory in front of the ROCm headers, and -DDIVANS_HOST_SIMT, compiles a .hip file's KERNELS as plain C++: a launch
// runs the workgroups one after the other inside the calling process, every lane a fiber of tests/c/simt/simt.cpp, one lane at a
// time.  Cross-lane operations and __syncthreads park the lane; the lanes of a wave that wait at the same call site are the exec mask
// the operation is carried out for.  LDS is one exact-size allocation per workgroup, a buffer resource keeps its num_records, and an
// access outside either ends the program with a finding.  The runtime's HOST API (streams, memory, errors) is the real header's, so
// the objects link with host code built by hipcc and with tests/c/fakehip_rt.cpp.  hipcc never sees this file.
#ifndef DIVANS_TESTS_SIMT_HIP_RUNTIME_H_
#define DIVANS_TESTS_SIMT_HIP_RUNTIME_H_
#ifndef DIVANS_HOST_SIMT
#error "tests/c/simt stands in for <hip/hip_runtime.h> only in a -DDIVANS_HOST_SIMT build"
#endif
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <functional>

#undef __global__
#undef __device__
#undef __host__
#undef __shared__
#undef __forceinline__
#undef __launch_bounds__
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))      // every inlined copy of a cross-lane operation is a call site of its own, as on the device
#define __launch_bounds__(...)

namespace simt {

struct Idx { uint32_t x, y, z; };
struct LaneIds { Idx thread, block, block_dim, grid_dim; };
const LaneIds& ids();              // of the lane that is running

// ---- findings ----------------------------------------------------------------------------------------------------------------
// prints "SIMT FINDING: kernel <name>, workgroup <w>, lane <l>: <what>" and aborts
[[noreturn]] void finding(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

// ---- LDS -----------------------------------------------------------------------------------------------------------------------
// The workgroup's dynamic LDS: exactly the launch's bytes, filled with the poison byte, at LDS address 0.  Pointers into it are
// checked by AddressSanitizer, 32-bit LDS addresses by lds_at().
uint8_t* dynamic_lds();
uint8_t* static_lds(const char* file, int line, size_t bytes);     // a function-local __shared__ array: one exact-size allocation per workgroup
uint32_t lds_addr(const void* p);                                   // the LDS address of a pointer into the dynamic LDS
uint8_t* lds_at(uint32_t addr, uint32_t bytes);                     // a finding unless [addr, addr + bytes) lies inside the dynamic LDS
// The accessors for 32-bit LDS addresses are carried out in lockstep, like the cross-lane operations below: the lanes of a wave that
// wait at the same access perform it together (all reads of one instruction before any write of the next), as a wave does.  A tag
// word that sixteen lanes read and then rewrite is read by all of them first.
uint32_t lds_read8(uint32_t a) __attribute__((noinline));
uint32_t lds_read16(uint32_t a) __attribute__((noinline));
uint32_t lds_read32(uint32_t a) __attribute__((noinline));
void lds_write16(uint32_t a, uint32_t v) __attribute__((noinline));
void lds_write32(uint32_t a, uint32_t v) __attribute__((noinline));

// ---- buffer resources ------------------------------------------------------------------------------------------------------------
struct BufferRsrc { uint8_t* base; uint32_t num_records; };
inline BufferRsrc make_buffer_rsrc(void* p, int stride, int num_records, int) {
    if (stride != 0) finding("buffer resource with stride %d: only raw buffers are modelled", stride);
    return BufferRsrc{(uint8_t*)p, (uint32_t)num_records};
}
// a finding unless [off, off + bytes) lies below num_records; the access itself is a plain one (AddressSanitizer sees the allocation)
uint8_t* buffer_at(const BufferRsrc& r, uint32_t off, uint32_t bytes, const char* what);
inline uint16_t buffer_load_b16(const BufferRsrc& r, uint32_t voff, uint32_t soff) { uint16_t v; memcpy(&v, buffer_at(r, voff + soff, 2, "load"), 2); return v; }
inline void buffer_store_b16(uint16_t v, const BufferRsrc& r, uint32_t voff, uint32_t soff) { memcpy(buffer_at(r, voff + soff, 2, "store"), &v, 2); }
template <class V> inline void buffer_store_b128(V v, const BufferRsrc& r, uint32_t voff, uint32_t soff) {
    static_assert(sizeof(V) == 16, "a 128-bit store");
    memcpy(buffer_at(r, voff + soff, 16, "store"), &v, 16);
}

// ---- cross-lane operations (wave64) ----------------------------------------------------------------------------------------------
// Each parks the calling lane until every live lane of its wave is parked; the lanes parked at the same return address form the exec
// mask.  A source lane outside the exec mask reads as an out-of-row one: 0 under bound_ctrl, `old` otherwise.
int dpp(int old, int src, int ctrl, bool bound_ctrl) __attribute__((noinline));
int bpermute(int byte_addr, int v) __attribute__((noinline));       // a source lane outside the exec mask reads 0
int readfirstlane(int v) __attribute__((noinline));
unsigned long long ballot(bool pred) __attribute__((noinline));
int shfl_xor(int v, int lane_mask) __attribute__((noinline));
void wave_sync() __attribute__((noinline));                         // the wave's lanes meet (a fence or wait: what lanes stored before it, the others see after it)
void syncthreads() __attribute__((noinline));                       // every live lane of the workgroup

// ---- launches ------------------------------------------------------------------------------------------------------------------
hipError_t launch(const void* kernel, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, const std::function<void()>& body);
}  // namespace simt

#define threadIdx (::simt::ids().thread)
#define blockIdx (::simt::ids().block)
#define blockDim (::simt::ids().block_dim)
#define gridDim (::simt::ids().grid_dim)

#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) \
    (void)::simt::launch((const void*)(kernel), (grid), (block), (lds), (stream), [=]() { (kernel)(__VA_ARGS__); })

// intrinsics: the 24-bit multiplies take the low 24 bits of their operands, as v_mul_i32_i24 / v_mul_u32_u24 do
inline int __mul24(int a, int b) { return (int)(uint32_t)((int64_t)((int32_t)((uint32_t)a << 8) >> 8) * (int64_t)((int32_t)((uint32_t)b << 8) >> 8)); }
inline uint32_t __umul24(uint32_t a, uint32_t b) { return (uint32_t)((uint64_t)(a & 0xffffffu) * (uint64_t)(b & 0xffffffu)); }
inline int __clz(int v) { return v == 0 ? 32 : __builtin_clz((unsigned)v); }
#define __ballot(p) ::simt::ballot((p) != 0)
#define __syncthreads() ::simt::syncthreads()
#define __shfl_xor(v, m) ::simt::shfl_xor((int)(v), (int)(m))
// atomics are plain: one lane runs at a time
template <class T, class U> inline T atomicOr(T* p, U v) { const T old = *p; *p = (T)(old | (T)v); return old; }
template <class T, class U> inline T atomicAdd(T* p, U v) { const T old = *p; *p = (T)(old + (T)v); return old; }

#define __builtin_amdgcn_mov_dpp(v, ctrl, row_mask, bank_mask, bound_ctrl) ::simt::dpp((v), (v), (ctrl), (bound_ctrl))
#define __builtin_amdgcn_update_dpp(old, v, ctrl, row_mask, bank_mask, bound_ctrl) ::simt::dpp((old), (v), (ctrl), (bound_ctrl))
#define __builtin_amdgcn_ds_bpermute(addr, v) ::simt::bpermute((addr), (v))
#define __builtin_amdgcn_readfirstlane(v) ::simt::readfirstlane((v))
#define __builtin_amdgcn_rcpf(x) (1.0f / (x))                       // the kernels' fix-ups absorb the difference to v_rcp_f32 (1 ulp)
#define __builtin_amdgcn_fence(order, scope) ::simt::wave_sync()
#define __builtin_amdgcn_s_waitcnt(n) ::simt::wave_sync()
#define __amdgpu_buffer_rsrc_t ::simt::BufferRsrc
#define __builtin_amdgcn_make_buffer_rsrc(p, stride, num, flags) ::simt::make_buffer_rsrc((p), (stride), (num), (flags))
#define __builtin_amdgcn_raw_buffer_load_b16(rsrc, voff, soff, aux) ::simt::buffer_load_b16((rsrc), (voff), (soff))
#define __builtin_amdgcn_raw_buffer_store_b16(v, rsrc, voff, soff, aux) ::simt::buffer_store_b16((v), (rsrc), (voff), (soff))
#define __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, voff, soff, aux) ::simt::buffer_store_b128((v), (rsrc), (voff), (soff))

#endif
