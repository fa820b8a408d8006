// mxe_shapes.h -- the shapes of the three chain kernels as the host needs them: the constants their LDS carves read and the
// bytes of dynamic LDS each build asks for.  Plain C++, no HIP: the kernels (mxe_kernel*.hip.h) and the planners (mxe_plan.h)
// include it, and tools/plan_dump.cpp evaluates it on the host.  Each formula restates the carve at the top of its kernel.
#pragma once
#include <cstddef>

#ifndef MXE_X_UL
#define MXE_X_UL 0            // chain_kernel_mc<.., 2>: u elements per lane kept in LDS instead of registers (0: all eight in registers)
#endif

namespace mxe {

constexpr int GRAM_R = 4;         // chain_kernel: rows staged per wave per Gram tile
constexpr int GBLK = 6;           //   staged doubles per 4-column block (16-B aligned, bank spread)
constexpr int LV_NWV = 8;         // chain_kernel_lv: wavefronts per workgroup
constexpr int LV_STATIC_LDS = 2304;     //   bound on the __shared__ arrays of the kernel (host side: fits-the-LDS test)
constexpr int LV_ACAP = 16;             //   alphas of a slot's piece kept in LDS: a laddered piece walks its rungs from that table only, so rungs + alphas
                                        //   of such a piece stay within it (emit_scan of mxe_plan.h); longer pieces read the scan's mesh from memory

// omega-space state of one workgroup of a GSTATE build of chain_kernel_mc, in doubles: u [nwp][4] | H [nwp][4] + look-ahead | sw [nwp][4] floats + look-ahead
constexpr int MC_GSTATE_PAD = 1024;
inline size_t mc_gstate_doubles(int nwp) { return (size_t)nwp * 4 + ((size_t)nwp * 4 + MC_GSTATE_PAD) + ((size_t)nwp * 4 + MC_GSTATE_PAD) / 2; }

// dynamic LDS of chain_kernel_mc<NA, WGPC, .., NWV, GSTATE> in bytes (the carve at the top of the kernel)
inline size_t mc_lds_bytes(int NA, int nwp, int wgpc, int nwv = 4, bool gst = false)
{
    const int NT = NA / 16, NPAIR = NT * (NT + 1) / 2;
    if (gst) nwp = 0;                        // (u, H, sw in device memory: MCExtra::gstate)
    const size_t doubles = 8 * 4 * 64 + 2 * 64 + 64 * 4 + (wgpc == 2 ? 2 : nwv) * 4 * 64 + nwv * 32 + 2 * 4 * 64 +   // vectors, c, 1/c, step, h, sums, solve scales
                           (wgpc == 2 ? (size_t)MXE_X_UL * 256 + (size_t)nwp * 4 : (size_t)2 * nwp * 4) +
                           (size_t)4 * NPAIR * 256;                                                  // u, H, Gram tiles
    const size_t floats = (size_t)nwp * 4;                                              // sw
    return doubles * 8 + floats * 4;
}

// LDS bytes of chain_kernel<NW, NAB, TS>: stream arrays (u, ut, w, wt, Hs, vecs) in the stream
// type, the Gram staging area only in the binary64 build
// (gst: the five omega arrays live in device memory, KParams::gstate)
inline size_t lds_bytes(int NP, int nwp, int NW, bool f32, bool gst = false)
{
    const int SROW = (NP / 4) * GBLK;
    const size_t fixed = (size_t)NP * (NP + 1) + (NP == 64 ? 13 : 11) * (size_t)NP + (size_t)NW * NP + (size_t)NW * 8;
    const size_t stream = (gst ? 0 : 5 * (size_t)nwp) + NP;
    const size_t stage = f32 ? 0 : (size_t)NW * 2 * GRAM_R * SROW;
    return (fixed + stage) * 8 + stream * (f32 ? 4 : 8);
}

// rows of V^T chain_kernel_lv keeps: the 32 columns of the active block at least, a multiple of eight (row-pass unroll)
inline int lv_rows(int ns) { const int r = (ns + 7) & ~7; return r < 32 ? 32 : r; }
// its dynamic LDS in bytes (the carve at the top of the kernel)
inline size_t lv_lds_bytes(int ns, int nwp)
{
    const size_t S32 = (size_t)nwp + 4;
    const size_t stage = 4 * S32 * 4;                                   // H or sw of the four slots
    const size_t solve = 4 * 4 * 64 * 8;                                // rhs, z, two scale vectors (alias sw)
    return (size_t)lv_rows(ns) * S32 * 4 + (4 * 4 * 64 + 2 * 64 + 4 * 64 + 64) * 8 + 3 * 4 * 64 * 4 +
           stage + (stage > solve ? stage : solve) + 4 * 3 * 256 * 4;
}

}  // namespace mxe
