// lds_dma.h — the few device primitives every LDS-DMA kernel of the library is built from: buffer descriptors, the DMA
// instruction itself, counted waits and the LDS address cast (the u32x4 vector type they move is in common.h).  One definition each; the kernels say what they count.
#pragma once
#include "common.h"

namespace mi {

// LDS byte address of a __shared__ object (address space 3 pointers are 32 bits wide)
__device__ __forceinline__ unsigned lds_addr(const void* p) {
    return (unsigned)(unsigned long)(const __attribute__((address_space(3))) void*)p;
}

// Raw buffer descriptor over [base, base + bytes).  The flags word 0x00020000 is DATA_FORMAT = 32 bits and nothing else: no
// stride (num_records counts BYTES and the range check is on the byte offset), no swizzle, no index — an access whose offset
// lies outside [0, bytes) as an unsigned number reads zeros / writes nothing.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000);
}

// LDS-DMA of 16 bytes per lane through a buffer descriptor (buffer_load_dwordx4 ... offen lds): lane i's 16 bytes at byte
// offset voff (per lane) go to LDS byte lds_dst + 16 i (lds_dst wave-uniform).  For offsets outside [0, num_records) the
// hardware range check writes ZEROS: row tails and dummy chunks need no select.
// Inline asm, so that hipcc does not see an LDS write: for the builtin forms (global_load_lds and buffer_load ... lds alike)
// it puts s_waitcnt vmcnt(0) in front of the next ds_read, which drains the ring every chunk (seen in the ISA of gemm_sk.hip;
// it knows nothing of the counted inline-asm waits below).  M0 carries the LDS address and is saved / restored around the
// instruction (cdna_hip_programming.md 5.7); the s_nop covers the M0 write -> LDS-DMA hazard.
template <typename RSRC>
__device__ __forceinline__ void dma16_buf(RSRC rsrc, int voff, unsigned lds_dst) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(lds_dst) : "memory");
#endif
}

// 16-byte store to global memory, write-through when `wt` (wave-uniform) is set: global_store_dwordx4 ... sc1, the policy of
// gemm_sk.hip's __builtin_amdgcn_raw_buffer_store_b128(..., 16) without a descriptor (the 64-bit address is the VGPR pair the plain
// store would use, so the register budget does not move).  A plain store leaves its line dirty in the XCD's L2 until the kernel
// boundary writes it back with every CU idle; an sc1 store sends the bytes on at once and drops the line, so a layer's output
// leaves under the epilogue's LDS hops instead of behind the last wave (MI355X_MICROARCH.md: store flavours, "boundary",
// "publish-large").  Only worth it when a wave instruction covers whole 128-byte lines.  Nothing in the storing launch may read
// the bytes back; the next launch sees them at the stream's kernel boundary as it does plain stores.  Inline asm: the compiler
// has no sc1 on an ordinary store; gfx9 stores read their data at issue, so no wait is owed before the registers are reused.
template <typename V>
__device__ __forceinline__ void store16(void* dst, const V& v, bool wt) {
    static_assert(sizeof(V) == 16, "store16: one dwordx4");
#if defined(__HIP_DEVICE_COMPILE__)
    if (wt) {
        u32x4 w;
        __builtin_memcpy(&w, &v, 16);
        asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(dst), "v"(w));
    } else {
        *reinterpret_cast<V*>(dst) = v;
    }
#endif
}

// counted waits: at most N of this wave's operations of that counter still in flight.  vmcnt: vector-memory loads (LDS-DMA
// included) return in order, so "all but the N youngest have landed" is exact.  lgkmcnt: LDS operations complete in order, but
// scalar memory loads share the counter and return OUT of order — a wait_lgkm<N > 0>() is exact only where no scalar load can be
// in flight (gemm_ph8.hip and gemm_x3d.hip count LDS reads behind a point where every kernel argument has arrived); anywhere
// else use wait_lgkm<0>().
template <int N> __device__ __forceinline__ void wait_vm() {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
#endif
}
template <int N> __device__ __forceinline__ void wait_lgkm() {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(N >= 0 && N < 16, "lgkmcnt is a 4-bit counter");
    asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(N) : "memory");
#endif
}

}  // namespace mi
