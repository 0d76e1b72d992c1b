// fp4_bits.h — presence bits as FP4 (E2M1) operands of gfx950's block-scaled MFMA, shared by the kinship Gram kernel
// (kin_kernels.hip) and the LD kernel (ld_kernels.hip).
//
// A nibble with only bit 0, 1 or 2 set is 0.5, 1.0 or 2.0 in E2M1, so `dword & (0x11111111 << j)` turns every fourth bit of a
// dword of presence bits into eight FP4 values in ONE lane-op; the operands' block scales (2^(1-j), exact) make every product
// of two set bits exactly 1.0. Bit 3 of a nibble is the FP4 sign: it is moved down first. v_mfma_scale_f32_16x16x128_f8f6f4
// accumulates those products in float32, exact below 2^24 of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef KGWAS_KIN_ABLATE
#define KGWAS_KIN_ABLATE 0
#endif

namespace kgwas {

typedef int kin_i32x4 __attribute__((ext_vector_type(4)));
typedef int kin_i32x8 __attribute__((ext_vector_type(8)));
typedef float kin_f32x4 __attribute__((ext_vector_type(4)));

// FP4 operand of MFMA step j = 0..3 from four plane dwords (128 rows of one sample): nibble e of operand dword q is
// bit 4e + j of plane dword q, i.e. k-element 8q + e <-> row 32q + 4e + j of the lane's 128 (A and B operands use the
// same map, so the k index pairs a row with itself). Steps 0..2 are one AND per dword (values 0.5, 1, 2: the block
// scale 2^(1-j) makes them 1), step 3 moves the FP4 sign bit down first (value 2, scale 2^-1).
__device__ __forceinline__ kin_i32x8 kin_expand_step(const uint4& w, int j) {
    kin_i32x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
    if (KGWAS_KIN_ABLATE & 32) {  // experiments: no expansion work
        r[0] = (int)w.x;
        r[1] = (int)w.y;
        r[2] = (int)w.z;
        r[3] = (int)w.w;
        return r;
    }
    if (j < 3) {
        const uint32_t mk = 0x11111111u << j;
        r[0] = (int)(w.x & mk);
        r[1] = (int)(w.y & mk);
        r[2] = (int)(w.z & mk);
        r[3] = (int)(w.w & mk);
    } else {
        r[0] = (int)((w.x >> 1) & 0x44444444u);
        r[1] = (int)((w.y >> 1) & 0x44444444u);
        r[2] = (int)((w.z >> 1) & 0x44444444u);
        r[3] = (int)((w.w >> 1) & 0x44444444u);
    }
    return r;
}

}  // namespace kgwas
