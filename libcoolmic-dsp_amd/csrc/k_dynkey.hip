// k_dynkey.hip -- gfx950 (MI355X, wave64) dynamics stage with side-chain keys: the level of stream key[s] steers the gain
// of stream s (ducking, linked stems; include/coolmic_hip.h, "dynamics", has the arithmetic to the bit).  Only the
// detector's input changes:
//     e = max_c |x_k[n][c]|, k = key[s]            L, l, g = curve_s(l), s and y = (x_s[n-D] * s[n] + 2^14) >> 15 as before
//
//   k_dynk_fast<C>  C in {1, 2}
//   k_dynk_any      3..16 channels
//   k_dynk_set      writes the key of a range of streams into the map, uint32 [S]; the key is a kernel argument
//
// The decomposition is k_dyn.hip's and the body is csrc/k_dyn.h's with KEYED = true.  A workgroup reads key[s] once,
// before anything else; step 1's loads then depend on it and on kernel arguments alone, and the curve still follows
// them.  Step 1 reads the key's run slot and the key's history slot: both hold raw input frames, the history in the slot
// the host's parity selects for reading, which no workgroup of the run writes -- so a tile of s may read the history of k
// while k's last tile writes k's other slot.  The delayed re-read, the history write, the copy of a stream without
// frames, the curve and the meter are stream s's own.  A keyed stream and its key have the same count (cmhip_dyn_run
// refuses a run otherwise), so the count of s bounds the loads from k.  The plan, the LDS and the grid are k_dyn.hip's.
// An object whose map holds no key never launches these kernels: cmhip_dyn_run picks k_dyn.hip's.
#include "k_dyn.h"

namespace cmhip {

template <int C>
__global__ __launch_bounds__(DYN_BLOCK) void k_dynk_fast(DynArgs a, const u32 *key)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<C, true>(a, key, reinterpret_cast<u32 *>(dyn_lds), cv, red);
}

__global__ __launch_bounds__(DYN_BLOCK) void k_dynk_any(DynArgs a, const u32 *key)
{
    extern __shared__ u32x4 dyn_lds[];
    __shared__ u32 cv[DYN_CURVE];
    __shared__ u32 red[4];
    dyn_tile<0, true>(a, key, reinterpret_cast<u32 *>(dyn_lds), cv, red);
}

// the key of streams first .. first + count - 1: `key`, or each stream itself where own != 0
__global__ __launch_bounds__(DYN_BLOCK) void k_dynk_set(u32 *map, u32 first, u32 count, u32 key, u32 own)
{
    const u32 i = blockIdx.x * DYN_BLOCK + threadIdx.x;
    if (i < count)
        map[first + i] = own ? first + i : key;
}

// ---------------------------------------------------------------------------
// launcher

hipError_t launch_dynk(const DynArgs &a, const uint32_t *key, hipStream_t st)
{
    const DynPlan p = plan_dyn(a.streams, a.channels, a.a, a.b, a.W - (1u << a.b), a.frames);
    if (p.grid == 0)
        return p.err ? hipErrorInvalidValue : hipSuccess;
    DynArgs b = a;
    b.halo = p.halo;
    b.chunks = p.chunks;
    b.tile_frames = p.tile_frames;
    switch (a.channels) {
    case 1: hipLaunchKernelGGL((k_dynk_fast<1>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b, key); break;
    case 2: hipLaunchKernelGGL((k_dynk_fast<2>), dim3(p.grid), dim3(p.block), p.lds_bytes, st, b, key); break;
    default: hipLaunchKernelGGL(k_dynk_any, dim3(p.grid), dim3(p.block), p.lds_bytes, st, b, key); break;
    }
    return hipGetLastError();
}

hipError_t launch_dyn_set_key(uint32_t *map, uint32_t first, uint32_t count, uint32_t key, bool own, hipStream_t st)
{
    if (count == 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_dynk_set, dim3((count + DYN_BLOCK - 1u) / DYN_BLOCK), dim3(DYN_BLOCK), 0, st, map, first, count,
                       key, own ? 1u : 0u);
    return hipGetLastError();
}

}  // namespace cmhip
