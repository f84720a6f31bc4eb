// The frame of the transposing slice-loop passes: what every rowT*_pass_kernel does AROUND its transform.  A kernel is its tables,
// its line layout (line_of / line_ptr) and its transform program; the job, the walk over the work items, the t_k row and the
// natural-order transposed store are here, once.  Force-inlined device pieces only, no kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "kernel_util.h"

// Ablation switches of tools/rowt_bench.hip (timing experiments on this pass; wrong results): 1 = no prefetch loads, 2 = no
// global stores (the tile reads stay), 4 = no lane <-> register exchanges, 8 = no transforms at all, 16 = one table entry instead
// of the table reads (the Fresnel factors and the twiddles that are not kept in registers), 32 = no tile write / barriers / store phase; rowTW_pass_kernel alone: 64 = no store phase, 128 = no tile write.  Never set in the library.
#ifndef MSL_ABL2
#define MSL_ABL2 0
#endif

namespace msl {

enum { P2_PRE_A = 1, P2_POST_A = 2, P2_POST_F = 4, P2_IN_PAIRED = 8, P2_OUT_PAIRED = 16 };

struct RowTJob {
    const float2* in;       // (P, n_lines, in_pitch): lines along the transform axis
    float2* out;            // (P, N, out_pitch): transposed
    const float2* trans;    // t_k in the input orientation, (n_lines, N) unpadded
    const float2* pl;       // (N) Fresnel factor along the line axis, 1/N folded in (split order for N = 2R^2)
    const float2* tw;
    const float2* tw2;      // N = 2R^2 only: W_N^m, m < R^2
    long long in_image_stride, out_image_stride;
    int in_pitch, out_pitch, n_lines, n_images, flags, pchunk;
    int t_group;            // frame batching: images [g t_group, (g+1) t_group) use the stack trans + g t_stride (0: one stack)
    unsigned t_magic;       // floor(2^32 / t_group) + 1
    long long t_stride;
    // rowTB_pass_kernel (lines of any length N <= R^2/2 by Bluestein's chirp-z on the register FFTs of length M = R^2):
    const float2* bf;       // (M/2 + 1) filter FFT_M(conj chirp, wrapped) / M -- an even sequence, first half stored
    const float2* bw;       // (M/2) chirp w[n] = exp(-i pi n^2 / N), zero for n >= N
    int n_line;             // N
    int perm_shift;         // rowT_pass_kernel<.., OUT_P>: log2(R' / 8), R' = radix of the kernel that reads the output lines
#ifdef MSL_CLOCK
    unsigned long long* clk;    // tools/rowt_bench.hip -DMSL_CLOCK: per workgroup, shader cycles and 100 MHz ticks spent in the item loop
#endif
};

// transmission stack of the frame that image p belongs to: job.trans + frame_off(job, p).  p is wave-uniform and the
// frame number p / t_group is computed in scalar registers only -- a multiply-high by t_magic = floor(2^32 / t_group) + 1,
// exact while p * t_group < 2^32 -- because these kernels run within a few VGPRs of the 256 that two waves per SIMD allow:
// a vector temporary here pushed rowT2_pass_kernel<16> into the AGPRs and halved its occupancy (81 -> 117 us per pass).
template <typename Job>
__device__ __forceinline__ long long frame_off(const Job& job, int p) {
    if (job.t_group <= 0) return 0;
    const unsigned up = (unsigned)__builtin_amdgcn_readfirstlane(p);
    const unsigned f = job.t_group == 1 ? up : __umulhi(up, job.t_magic);        // (the magic number of 1 does not fit 32 bits)
    return (long long)f * job.t_stride;
}

// The persistent workgroup's walk over its work items.  Work item = (line block lb, probe chunk pc), item = lb * pchunks + pc:
// a block of the kernel's LINES lines and a chunk of PC = job.pchunk images that share t_k, so the t_k lines stay in registers
// across the chunk; k counts the images of the chunk (the last chunk may be ragged).  Workgroup b takes items b, b + grid, ...
// The cursor (item, lb, pc, k) advances incrementally -- a division per iteration costs ~0.3 us of scalar work on the critical
// path.  Everything here is wave-uniform and stays in scalar registers, for the reason given at frame_off.
struct RowTCursor {
    int item, lb, pc, k;
    int PC, pchunks, n_items, step_lb, step_pc, n_images;       // of the launch

    // line_blocks: n_lines / LINES, rounded up in the kernels whose last tile may be ragged
    static __device__ __forceinline__ RowTCursor first(const RowTJob& job, int line_blocks) {
        RowTCursor c;
        c.PC = job.pchunk;
        c.n_images = job.n_images;
        c.pchunks = (job.n_images + c.PC - 1) / c.PC;
        c.n_items = line_blocks * c.pchunks;
        c.step_lb = (int)gridDim.x / c.pchunks; c.step_pc = (int)gridDim.x % c.pchunks;
        c.item = blockIdx.x;
        c.lb = c.item / c.pchunks; c.pc = c.item - c.lb * c.pchunks; c.k = 0;
        return c;
    }
    __device__ __forceinline__ bool valid() const { return item < n_items; }
    __device__ __forceinline__ int image() const { return pc * PC + k; }
    __device__ __forceinline__ int chunk_image() const { return pc * PC; }          // first image of the chunk: its frame is the chunk's
    __device__ __forceinline__ RowTCursor next() const {
        RowTCursor n = *this;
        if (++n.k >= min(PC, n_images - pc * PC)) {
            n.k = 0; n.item = item + (int)gridDim.x; n.lb = lb + step_lb; n.pc = pc + step_pc;
            if (n.pc >= pchunks) { n.pc -= pchunks; ++n.lb; }
        }
        return n;
    }
    // what an unconditional prefetch reads during this item: the line of nxt = next(), past the last item the current line again
    __device__ __forceinline__ RowTCursor prefetch_target(const RowTCursor& nxt) const {
        const bool more = nxt.valid();
        RowTCursor c = *this;
        c.lb = more ? nxt.lb : lb; c.pc = more ? nxt.pc : pc; c.k = more ? nxt.k : k;
        return c;
    }
};

// t_k row of input line `line` (n points per line) for the chunk of c: fetched when c.k == 0, kept in registers across the chunk
__device__ __forceinline__ const float2* rowt_trans_row(const RowTJob& job, const RowTCursor& c, int line, int n) {
    return job.trans + frame_off(job, c.chunk_image()) + (long long)line * n;
}
// output image of c (transposed: position e of line l at e * out_pitch + l)
__device__ __forceinline__ float2* rowt_out_image(const RowTJob& job, const RowTCursor& c) {
    return job.out + (long long)c.image() * job.out_image_stride;
}

// The natural-order transposed store of a tile of LINES lines (row pitch CS float2, position e of a line at pos_map(e)) by NT
// threads: dst = the output image at the tile's first line, positions [0, NPOS) of which those below n_valid exist when GUARD.
// A thread stores two neighbouring lines of one position, 16 bytes; LINES / 2 threads make a segment of LINES * 8 bytes.
// Between two lds_barrier() of the caller.  STREAM: non-temporal store (a plain one where that measured faster).
struct PosIdentity { __device__ __forceinline__ int operator()(int e) const { return e; } };
template <int LINES, int NT, int CS, int NPOS, bool GUARD, bool STREAM, typename PosMap = PosIdentity>
__device__ __forceinline__ void tile_store_transposed(const float2* tile, float2* dst, int out_pitch, int n_valid, int tid, PosMap pos_map = PosMap{}) {
    constexpr int TPS = LINES / 2;                    // threads (16 B = 2 lines each) per output segment
    constexpr int POS_PER_IT = NT / TPS;
    constexpr int NIT = (NPOS + POS_PER_IT - 1) / POS_PER_IT;
    const int q = tid % TPS, r0 = tid / TPS;
    // uniform 64-bit base + per-thread 32-bit element offset, re-derived every iteration (the asm keeps the
    // compiler from hoisting 16 loop-invariant 64-bit addresses into registers for the whole kernel)
    int off0 = 2 * q + r0 * out_pitch;
    asm volatile("" : "+v"(off0));
    const int ostep = POS_PER_IT * out_pitch;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int pos = r0 + POS_PER_IT * i;
        if (!GUARD || pos < n_valid) {
            const float2 a = tile[(2 * q) * CS + pos_map(pos)], b = tile[(2 * q + 1) * CS + pos_map(pos)];
#if MSL_ABL2 & 2
            if (a.x == 1.2345e-30f)                 // never true: the LDS reads stay, the store goes
#endif
            {
                if constexpr (STREAM) st_stream(dst + (off0 + i * ostep), a.x, a.y, b.x, b.y);
                else *reinterpret_cast<float4*>(dst + (off0 + i * ostep)) = make_float4(a.x, a.y, b.x, b.y);
            }
        }
    }
}

}  // namespace msl
