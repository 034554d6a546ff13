// sha256_device.hpp — SHA-256 (FIPS 180-4) building blocks for gfx950 (CDNA4),
// for the BitTorrent v2 (BEP 52) merkle kernels in sha256_kernels.hip.
//
// Same idiom as sha1_device.hpp, pure 32-bit integer VALU work:
//   rotr            -> v_alignbit_b32
//   Σ0/Σ1/σ0/σ1     -> 2-3 alignbit/shift + one v_bitop3_b32 (xor of three)
//   Ch, Maj         -> one v_bitop3_b32 each
//   5-way add       -> v_add3_u32 (K[t] rides in an SGPR: gfx9 VOP3 takes no literal)
//   bswap           -> v_perm_b32
// Per round: 6 alignbit + 2 xor3 + Ch + Maj + 4 adds; per scheduled word
// 4 alignbit/shift + 2 xor3 + 2 adds.  No MFMA: bitwise work, not a contraction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vx {
namespace sha256 {

constexpr uint32_t kK[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};

constexpr uint32_t kIv[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                             0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};

// K[t] + W[t] of a block known at compile time (the padding block of a
// message whose length is a multiple of 64): the whole message schedule folds
// into 64 constants and the block costs its rounds only.
struct ConstBlock {
    uint32_t kw[64];
};

constexpr uint32_t c_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// The padding block that follows `bytes` message bytes, bytes % 64 == 0:
// 0x80, zeros, the 64-bit bit count.
constexpr ConstBlock pad_block(uint64_t bytes) {
    uint32_t w[64] = {};
    w[0] = 0x80000000u;
    w[14] = (uint32_t)((bytes * 8) >> 32);
    w[15] = (uint32_t)(bytes * 8);
    for (int t = 16; t < 64; ++t) {
        const uint32_t s0 = c_rotr(w[t - 15], 7) ^ c_rotr(w[t - 15], 18) ^ (w[t - 15] >> 3);
        const uint32_t s1 = c_rotr(w[t - 2], 17) ^ c_rotr(w[t - 2], 19) ^ (w[t - 2] >> 10);
        w[t] = w[t - 16] + s0 + w[t - 7] + s1;
    }
    ConstBlock b{};
    for (int t = 0; t < 64; ++t) b.kw[t] = w[t] + kK[t];
    return b;
}

__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }

// v_bitop3_b32 truth tables with src0=0xF0, src1=0xCC, src2=0xAA.
#define VX256_CH(e, f, g) __builtin_amdgcn_bitop3_b32((e), (f), (g), 0xCA)
#define VX256_MAJ(a, b, c) __builtin_amdgcn_bitop3_b32((a), (b), (c), 0xE8)
#define VX256_XOR3(a, b, c) __builtin_amdgcn_bitop3_b32((a), (b), (c), 0x96)

__device__ __forceinline__ uint32_t big_sigma0(uint32_t x) { return VX256_XOR3(rotr(x, 2), rotr(x, 13), rotr(x, 22)); }
__device__ __forceinline__ uint32_t big_sigma1(uint32_t x) { return VX256_XOR3(rotr(x, 6), rotr(x, 11), rotr(x, 25)); }
__device__ __forceinline__ uint32_t small_sigma0(uint32_t x) { return VX256_XOR3(rotr(x, 7), rotr(x, 18), x >> 3); }
__device__ __forceinline__ uint32_t small_sigma1(uint32_t x) { return VX256_XOR3(rotr(x, 17), rotr(x, 19), x >> 10); }

struct State {
    uint32_t h[8];
};

__device__ __forceinline__ State iv() {
    return State{{kIv[0], kIv[1], kIv[2], kIv[3], kIv[4], kIv[5], kIv[6], kIv[7]}};
}

#define VX256_ROUND(kw)                                               \
    do {                                                              \
        const uint32_t t1 = h + big_sigma1(e) + VX256_CH(e, f, g) + (kw); \
        const uint32_t t2 = big_sigma0(a) + VX256_MAJ(a, b, c);       \
        h = g;                                                        \
        g = f;                                                        \
        f = e;                                                        \
        e = d + t1;                                                   \
        d = c;                                                        \
        c = b;                                                        \
        b = a;                                                        \
        a = t1 + t2;                                                  \
    } while (0)

// Compress one block; w[] holds the 16 big-endian message words and is used
// as the rolling schedule buffer (clobbered).
__device__ __forceinline__ void compress(State& s, uint32_t (&w)[16]) {
    uint32_t a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
#pragma unroll
    for (int t = 0; t < 64; ++t) {
        uint32_t wt;
        if (t < 16) {
            wt = w[t];
        } else {
            wt = small_sigma1(w[(t - 2) & 15]) + w[(t - 7) & 15] + small_sigma0(w[(t - 15) & 15]) + w[t & 15];
            w[t & 15] = wt;
        }
        VX256_ROUND(kK[t] + wt);
    }
    s.h[0] += a;
    s.h[1] += b;
    s.h[2] += c;
    s.h[3] += d;
    s.h[4] += e;
    s.h[5] += f;
    s.h[6] += g;
    s.h[7] += h;
}

// Compress a block known at compile time (pad_block): rounds only.
__device__ __forceinline__ void compress_const(State& s, const ConstBlock& blk) {
    uint32_t a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
#pragma unroll
    for (int t = 0; t < 64; ++t) VX256_ROUND(blk.kw[t]);
    s.h[0] += a;
    s.h[1] += b;
    s.h[2] += c;
    s.h[3] += d;
    s.h[4] += e;
    s.h[5] += f;
    s.h[6] += g;
    s.h[7] += h;
}

__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

// Compress the 64-byte block held little-endian in four uint4 registers.
__device__ __forceinline__ void compress_le(State& s, const uint4& q0, const uint4& q1, const uint4& q2,
                                            const uint4& q3) {
    uint32_t w[16] = {bswap(q0.x), bswap(q0.y), bswap(q0.z), bswap(q0.w), bswap(q1.x), bswap(q1.y),
                      bswap(q1.z), bswap(q1.w), bswap(q2.x), bswap(q2.y), bswap(q2.z), bswap(q2.w),
                      bswap(q3.x), bswap(q3.y), bswap(q3.z), bswap(q3.w)};
    compress(s, w);
}

}  // namespace sha256
}  // namespace vx
