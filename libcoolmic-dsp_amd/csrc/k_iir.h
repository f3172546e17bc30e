// k_iir.h -- what the filter's two kernel files share (k_iir.hip, k_iirramp.hip): the tile between the slots and LDS,
// a section's five words from the table, and the counters' add.  The step itself -- iir_input, iir_section, iir_output
// -- is csrc/iir_plan.h's, which the host tests compile too.
#ifndef CMHIP_K_IIR_H
#define CMHIP_K_IIR_H

#include "cmhip_device.h"

namespace cmhip {

constexpr u32 IIR_LDS_SAMPLES = IIR_BLOCK * IIR_TILE + 2u * IIR_BLOCK;     // spw * C <= 64 rows of B samples, and the pitch's pad
constexpr u32 IIR_UNROLL = 4;                                    // frames whose LDS reads, and then writes, go together

// The workgroup's tile t between the slots and LDS: spw * B C / 8 <= 512 vectors, lane l takes the vectors l + 64 q,
// q < IIR_MOVE.  Vector i of the workgroup: IirVec, its stream, its place in LDS -- 4-byte aligned there, for the
// streams' tiles lie iir_lds_pitch apart: a vector is four dwords to LDS.
constexpr u32 IIR_MOVE = IIR_TILE / 8u;                          // 8 vectors per lane at most

struct IirMove {
    IirVec v;
    u32 s;
    u32 at;                                          // its first sample in LDS
    bool mine;                                       // the vector exists and its stream does
};
__device__ __forceinline__ IirMove iir_move_at(const IirArgs &a, u32 s0, u32 spw, u32 C, u32 t, u32 q)
{
    const u32 nv = iir_tile_vecs(C), i = threadIdx.x + IIR_BLOCK * q;
    const u32 j = i / nv;
    IirMove m;
    m.s = s0 + j;
    m.at = j * iir_lds_pitch(C) + (i - j * nv) * 8u;
    m.mine = j < spw && m.s < a.streams;
    m.v = IirVec{0, 0};
    if (m.mine)
        m.v = iir_tile_vec(a.counts[m.s], C, t, i - j * nv);
    return m;
}

// the whole vectors of tile t on their way into registers: issued together, and a tile ahead of their use
__device__ __forceinline__ void iir_tile_fetch(const IirArgs &a, u32x4 (&r)[IIR_MOVE], u32 s0, u32 spw, u32 C, u32 t)
{
#pragma unroll
    for (u32 q = 0; q < IIR_MOVE; q++) {
        const IirMove m = iir_move_at(a, s0, spw, C, t, q);
        r[q] = u32x4{0, 0, 0, 0};
        if (m.mine && m.v.n == 8u)
            r[q] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(a.in + (u64)m.s * a.in_stride + m.v.off));
    }
}

// ... and into LDS; a vector that the stream's count cuts is read here, sample by sample
__device__ __forceinline__ void iir_tile_commit(const IirArgs &a, const u32x4 (&r)[IIR_MOVE], int16_t *lds, u32 s0, u32 spw,
                                                u32 C, u32 t)
{
#pragma unroll
    for (u32 q = 0; q < IIR_MOVE; q++) {
        const IirMove m = iir_move_at(a, s0, spw, C, t, q);
        int16_t *l = lds + m.at;
        if (m.mine && m.v.n == 8u) {
            u32 *w = reinterpret_cast<u32 *>(l);
            w[0] = r[q].x; w[1] = r[q].y; w[2] = r[q].z; w[3] = r[q].w;
        } else if (m.mine) {
            const int16_t *g = a.in + (u64)m.s * a.in_stride + m.v.off;
            for (u32 k = 0; k < m.v.n; k++)
                l[k] = g[k];
        }
    }
}

// the tile from LDS to the output slots
__device__ __forceinline__ void iir_tile_store(const IirArgs &a, const int16_t *lds, u32 s0, u32 spw, u32 C, u32 t)
{
#pragma unroll
    for (u32 q = 0; q < IIR_MOVE; q++) {
        const IirMove m = iir_move_at(a, s0, spw, C, t, q);
        if (!m.mine)
            continue;
        const int16_t *l = lds + m.at;
        int16_t *g = a.out + (u64)m.s * a.out_stride + m.v.off;
        if (m.v.n == 8u) {
            const u32 *w = reinterpret_cast<const u32 *>(l);
            const u32x4 o = {w[0], w[1], w[2], w[3]};
            __builtin_nontemporal_store(o, reinterpret_cast<u32x4 *>(g));
        } else
            for (u32 k = 0; k < m.v.n; k++)
                g[k] = l[k];
    }
}

__device__ __forceinline__ IirSec iir_load_sec(const int32_t *p) { return {p[0], p[1], p[2], p[3], p[4]}; }

__device__ __forceinline__ void iir_count(unsigned long long *where, u64 n)
{
    if (n)
        atomicAdd(where, n);
}

// the ramp kernels' launch (k_iirramp.hip): a.coef is the ramp table, IIR_RAMP_WORDS per section
void launch_iir_ramp(const IirArgs &a, const IirPlan &p, hipStream_t st);

}  // namespace cmhip
#endif
