// Shared declarations of the Winograd translation units (wino.hip: F(2x2,3x3); wino24.hip, wino24n.hip, wino24_wgrad.hip, wino24g.hip:
// F(2x4,3x3); wino44g.hip: F(4x4,3x3)): the parameter structs several kernels take, and the ONE host-side launch layer around them --
// tile geometry and partial-row rule, the tail of every forward launcher (wino_forward_plan + wino_dispatch), the split count of the
// in-kernel-transform weight gradients, the filter-pack launch, and the entry points of the two pre-transformed forms as one body over
// a WinoPreForm.  A translation unit keeps its kernels, its argument checks and the choice of its own template instantiation.
#pragma once
#include <stdio.h>
#include <algorithm>
#include <type_traits>
#include "common.hip.h"
#include "clamd_internal.h"

namespace clamd {

struct WinoParams {
    const float* x; int x_ldc;
    const float* w;              // [Kp/8][16 | 24][Np][8]
    const float* bias;
    float* y; int y_ldc;
    float* stats;                // partial rows [pixel tile][2][Np] (plain stores) or null
    int B, H, W, Kp, Np, relu;
    int band;                    // output-channel slabs per band of the block order (see clamd_conv3x3_winograd)
    int nblk;                    // (pixel tile, slab) pairs; the grid is min(nblk, CUs) persistent workgroups
    // forward launches behind a folded BatchNorm (clamd_bn_fold_bias): bias is a [9][Np] table indexed by the border class of the output pixel
    int bias_classes = 0;
};

// One filter-transform job = one GEMM operand: dst[(k/8)*P + xi][n][k%8] = (G g G^T)[xi] (P = 16 or 24 planes) with
// g = w[n_l][k_l] (forward) or the tap-flipped w[k_l][n_l] (data gradient); physical -> logical channel maps as in
// clamd_pack (two segments for concat inputs, zero padding).  One thread per (n, k).
struct WinoPackJob {
    const float* w; float* dst;
    int Np, Kp, N, K;                 // physical / logical sizes of the GEMM's N (rows) and K
    int n_seg0, n_seg0p, k_seg0, k_seg0p;
    int dgrad;                        // 0: g = w[n][k], src [N][K][3][3]; 1: g = flip(w[k][n]), src [K][N][3][3]
    int block0;                       // first workgroup of this job
    const float* kscale;              // optional [Kp]: g is multiplied by kscale[physical k] before the transform (bnfold.hip)
};

__device__ inline int wn_phys2log(int p, int seg0, int seg0p, int L) {
    if (p < seg0p) return p < seg0 ? p : -1;
    const int l = seg0 + (p - seg0p);
    return l < L ? l : -1;
}

// split-K reduce of every weight-gradient form: out[R][C][3][3] from the [nsplit] slabs in `partial`
struct WinoReduceParams {
    const float* partial; float* out;
    int nsplit, Rp, Cp, R, C, r_seg0, r_seg0p, c_seg0, c_seg0p;
};

// ---------------------------------------------------------------------------------------------------------------------
// host-side launch layer
// ---------------------------------------------------------------------------------------------------------------------
// records "<who>: <what>" (an entry point's name and its refusal) for clamd_last_error(); returns the negative status
inline int wino_fail(const char* who, const char* what) {
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return clamd_fail(msg);
}

// Pixels of a workgroup tile: `rows` x 32, or 2 `rows` x 16 for images narrower than 32 (32 Winograd tiles either way).
struct WinoTile { int ph, pw; };
inline WinoTile wino_tile(int W, int rows) { return W >= 32 ? WinoTile{rows, 32} : WinoTile{2 * rows, 16}; }
inline WinoTile w24_tile(int W) { return wino_tile(W, 8); }         // every F(2x4) forward kernel: 8 x 32 or 16 x 16 pixels
inline WinoTile w44_block(int W) { return wino_tile(W, 16); }       // F(4x4) tile block: 16 x 32 or 32 x 16 pixels
inline long long wino_tiles(WinoTile t, int B, int H, int W) { return (long long)B * ((H + t.ph - 1) / t.ph) * ((W + t.pw - 1) / t.pw); }

// partial statistics rows of a forward launch: one per pixel tile (one workgroup per tile and slab of `slab` output channels), or one
// per workgroup of the persistent grid (`wg_per_cu` on every usable CU)
inline long long wino_stat_rows(long long tiles, int Cout_p, int slab, int wg_per_cu, const clamd_tuning& tn) {
    const long long nblk = tiles * ((Cout_p + slab - 1) / slab), cap = (long long)wg_per_cu * clamd_usable_cus(tn);
    return (tn.wino_persist && nblk > cap) ? cap : tiles;
}

// block order of the forward kernels: output-channel slabs per band (HBM traffic model, wino.hip)
int wino_band(long long tiles, long long slabs, double x_elems, double f_elems, int forced);

// The tail of every forward launcher (wino.hip): refuses a grid out of range and a `stat_rows` other than `want_rows` (the answer of
// clamd_stat_rows(`op`, ...)) in the name of `who`; then p.band from the traffic model, p.nblk = tiles x slabs, the grid (persistent:
// at most `grid_cap` workgroups) and whether the image is no whole number of tiles `t` (a caller whose kernel handles a partial slab
// adds that term).  0 or the negative status.
struct WinoGrid { unsigned grid; bool ragged; };
int wino_forward_plan(WinoParams& p, WinoTile t, long long slabs, double x_elems, double f_elems, long long grid_cap, int stat_rows,
                      long long want_rows, const clamd_tuning& tn, const char* who, const char* op, WinoGrid* g);

// The forward launchers' choice among the instantiations of one kernel template: launch(wide, ragged, cls) is called with
// std::true_type / std::false_type arguments, so the caller's lambda names its kernel as <wide() ? 8 : 4, ragged(), cls()>
// (a template without the border-class parameter passes cls = false and ignores the third argument).
template <class F>
inline void wino_dispatch(bool wide, bool ragged, bool cls, F&& launch) {
    auto pick = [](bool b, auto&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); };
    pick(wide, [&](auto w) { pick(ragged, [&](auto r) { pick(cls, [&](auto c) { launch(w, r, c); }); }); });
}

// Split count of the in-kernel-transform weight gradients (clamd_wgrad_winograd, clamd_wgrad_winograd24) over `ntiles` pixel tiles and
// `blocks` output blocks (64 x 64 or 64 x 32 channels); *per = tiles per split.  wino_wgrad_max_split bounds it over every tuning.
int wino_wgrad_nsplit(int ntiles, int blocks, const clamd_tuning& tn, int* per);
inline int wino_wgrad_max_split(int blocks) { return std::max(1, 512 / blocks); }      // wgrad_blocks <= 1024 counts two per CU

// One launch of a fold-capable filter-pack kernel (wino_pack_kernel, wino24_pack_kernel): the job table's workgroups, and Cout_p more
// behind them for the border-class bias table of a folded BatchNorm (bnfold.hip)
using WinoPackKernel = void (*)(const WinoPackJob*, int, int, const FoldBias);
int wino_launch_pack(WinoPackKernel kernel, const char* who, const void* jobs_dev, int njobs, int total_blocks, const FoldBias* fold, hipStream_t stream);

#ifdef CLAMD_DIAG
// reader of a diagnostic build's __device__ counter array: copies it out and optionally clears it
#define CLAMD_DIAG_READER(fn_, sym_, n_)                                                                                   \
    int fn_(unsigned long long* out, int reset) {                                                                          \
        if (hipMemcpyFromSymbol(out, HIP_SYMBOL(sym_), 8 * (n_)) != hipSuccess) return -1;                                 \
        if (reset) { unsigned long long z[n_] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(sym_), z, 8 * (n_)) != hipSuccess) return -1; } \
        return 0;                                                                                                          \
    }
#endif

// wino24.hip
long long clamd_winograd24_stat_rows(int B, int H, int W, int Cout_p, const clamd_tuning& tn);
int launch_wino24(WinoParams p, const clamd_tuning& tn, int stat_rows, hipStream_t stream);
// wino44g.hip
long long clamd_winograd44_stat_rows(int B, int H, int W, int Cout_p, const clamd_tuning& tn);
// wino24n.hip: the same launch as half-width workgroups (32 tiles x 32 channels, two per CU; clamd_tuning::wino_half)
long long clamd_winograd24_half_stat_rows(int B, int H, int W, int Cout_p, const clamd_tuning& tn);
int launch_wino24_half(WinoParams p, const clamd_tuning& tn, int stat_rows, hipStream_t stream);

// ---------------------------------------------------------------------------------------------------------------------
// The two forms with pre-transformed operands, F(2x4) (wino24g.hip) and F(4x4) (wino44g.hip): one description each, one body per entry
// point (wino24g.hip).  Their checks differ only in what is listed here.
// ---------------------------------------------------------------------------------------------------------------------
struct WinoPreForm {
    const char* name;                    // "winograd24" / "winograd44" in every message
    const char* op;                      // the form's clamd_stat_rows op, as named in the stat_rows refusal
    const char* hw_rule;                 // the refusal of an image that is no whole number of output tiles ...
    const char* tile_note;               // ... and what the forward entry points append to it
    int planes;                          // 24 / 36 Winograd planes
    int hmask;                           // H & hmask must be 0 (W & 3 in both)
    WinoTile (*tile)(int W);
    int xform_wgs;                       // workgroups of the input transform per tile block
    double band_x;                       // transformed input per input element (wino_band's traffic model): 3.0 / 2.25
    int cin_mult, cin_min, y_mult;       // forward: Cin_p % cin_mult == 0, Cin_p >= cin_min, y_ldc % y_mult == 0
    bool y_bound;                        // forward: one output image must stay below 2^31 bytes
    const char* yt_launch;               // what a failed launch of the stand-alone gradient transform is reported as
    long long (*stat_rows)(int B, int H, int W, int Cout_p, const clamd_tuning& tn);
    // the form's own kernels: input transform, forward GEMM loop, gradient transform, split-K reduce (phs = 1, 2 or 4 split phases)
    void (*launch_xform)(bool wide, unsigned grid, hipStream_t s, const float* x, int x_ldc, const float* scale, const float* shift, float* v,
                         int B, int H, int W, int Cp);
    void (*launch_conv)(bool wide, bool ragged, unsigned grid, hipStream_t s, const WinoParams& p);
    void (*launch_yt)(bool wide, unsigned grid, hipStream_t s, const float* gz, int gz_ldc, float* yt, int B, int H, int W, int Rp, int Tp);
    void (*launch_reduce)(int phs, unsigned grid, hipStream_t s, const WinoReduceParams& p);
};
size_t wino_pre_input_elems(const WinoPreForm& f, int B, int H, int W, int Cp);
int wino_pre_transform_input(const WinoPreForm& f, const float* x, int x_ldc, const float* scale, const float* shift, float* v, int B, int H, int W,
                             int Cp, void* stream);
int wino_pre_conv3x3(const WinoPreForm& f, const float* v, const float* w_wino, const float* bias, float* y, int y_ldc, float* stats, int stat_rows,
                     int B, int H, int W, int Cin_p, int Cout_p, int relu, const clamd_tuning* tune, void* stream);
size_t wino_pre_operand_elems(const WinoPreForm& f, int B, int H, int W, int Rp);
size_t wino_pre_workspace_bytes(const WinoPreForm& f, int B, int H, int W, int Rp, int Cp);
int wino_pre_wgrad(const WinoPreForm& f, const float* gz, int gz_ldc, const float* v, float* yt, float* workspace, size_t ws_bytes, float* out,
                   int B, int H, int W, int Rp, int Cp, int R, int C, int r_seg0, int r_seg0p, int c_seg0, int c_seg0p, const clamd_tuning* tune,
                   void* stream);
int wino_pre_wgrad_transform(const WinoPreForm& f, const float* gz, int gz_ldc, float* yt, int B, int H, int W, int Rp, void* stream);

}  // namespace clamd
