// engine.hip — C-ABI entry points of librnnt_engine.so (see include/rnnt_engine.h).
//
// Host-side only: argument validation, workspace carving and kernel sequencing on the
// caller's stream.  No allocation, no synchronisation, no state kept between calls.
#include "../../include/rnnt_engine.h"

#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <dlfcn.h>
#include <string>

#include "kernels.hpp"
#include "mma_common.hpp"

namespace {

thread_local std::string g_err;
// The shipped library keeps NO mutable state besides the thread-local error string: kernel
// variants are selected per call (rnnt_engine_run_stages).  Only diagnostic builds
// (-DRNNT_ABLATE: in-kernel ablation switches; -DRNNT_STAMPS: s_memtime stamps) carry the
// process-wide words rnnt_engine_set_flags / rnnt_engine_set_debug write.
#if defined(RNNT_ABLATE) || defined(RNNT_STAMPS)
int g_flags = 0;
unsigned long long *g_debug = nullptr;
#else
constexpr int g_flags = 0;
constexpr unsigned long long *g_debug = nullptr;
#endif

}  // namespace

// record the calling thread's error message (rnnt_engine_last_error) and hand the code back
int engine_fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {
#define fail engine_fail

inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The control block of the fused workspace (rnnt_engine_ws_layout::counters): the one map of it, offset: member
struct ControlBlock {
    unsigned queue[128];       //    0: eight per-XCD work-item counters of the persistent dHidden kernel, 64 B apart
    unsigned fwd_tile[32];     //  512: tile counter of the persistent forwards
    float x2_scales[32];       //  640: f16x2 {s_W, 1 / s_W} (k_x2_wscale, every call)
    unsigned lattice_err[32];  //  768: error word of the lattice sweep
    unsigned ep_flag[32];      //  896: f16x2, != 0 when an input lies outside the factored tanh's range
    long *dw_tab() { return (long *)(this + 1); }  // 1024: dW live-row table, 2B + 2 longs, or the fp32 route's larger live-granule list (dw_list_bytes)
    static size_t dw_table_bytes(int B) { return align_up((2 * (size_t)B + 2) * 8); }
    int *dw_prog(int B) { return (int *)((char *)(this + 1) + dw_table_bytes(B)); }  // behind the table: [n_split][16] progress words of k_dw_bf16 / k_dw_x2
};
static_assert(sizeof(ControlBlock) == 1024 && offsetof(ControlBlock, fwd_tile) == 512 && offsetof(ControlBlock, x2_scales) == 640 &&
              offsetof(ControlBlock, lattice_err) == 768 && offsetof(ControlBlock, ep_flag) == 896, "control block map");

// The loss arrays and the dimensions of LatticeArgs (kernels.hpp), filled here for every caller: the standalone loss entries' workspace,
// denom_s | lpb_s | lpe_s | alpha_s | beta_s | coef | err (256 bytes), which layout() also places inside the fused one.  Returns its bytes.
size_t carve_loss_ws(void *workspace, int B, int T, int U1, LatticeArgs &a)
{
    const size_t skew = (size_t)B * ((size_t)T + U1 - 1) * U1, cells = (size_t)B * T * U1;
    const size_t s4 = align_up(skew * 4), s8 = align_up(skew * 8), co = 3 * s4 + 2 * s8, er = co + align_up(cells * 16);
    const uintptr_t p = (uintptr_t)workspace;
    a.denom_s = (float *)p; a.lpb_s = (float *)(p + s4); a.lpe_s = (float *)(p + 2 * s4); a.alpha_s = (double *)(p + 3 * s4);
    a.beta_s = (double *)(p + 3 * s4 + s8); a.coef = (CellCoef *)(p + co); a.err = (unsigned *)(p + er);
    a.B = B; a.T = T; a.U1 = U1; a.D = T + U1 - 1;
    return er + 256;
}

int check_dims(int B, int T, int U1, int H, int V, int dtype, bool need_h)
{
    if (dtype != RNNT_DTYPE_F32 && dtype != RNNT_DTYPE_BF16 && dtype != RNNT_DTYPE_F32_BF16X3 && dtype != RNNT_DTYPE_F32_F16X2)
        return fail(RNNT_ERR_UNSUPPORTED, "dtype %d not supported (RNNT_DTYPE_F32 / RNNT_DTYPE_BF16 / RNNT_DTYPE_F32_BF16X3 / RNNT_DTYPE_F32_F16X2)", dtype);
    const char *dname = dtype == RNNT_DTYPE_BF16 ? "RNNT_DTYPE_BF16" : dtype == RNNT_DTYPE_F32_F16X2 ? "RNNT_DTYPE_F32_F16X2" : "RNNT_DTYPE_F32_BF16X3";
    if (dtype != RNNT_DTYPE_F32 && !need_h)
        return fail(RNNT_ERR_UNSUPPORTED, "%s only applies to the fused joint+loss entry", dname);
    if (dtype != RNNT_DTYPE_F32 && (H <= 0 || H % 128 != 0 || V <= 0 || V % 128 != 0))
        return fail(RNNT_ERR_UNSUPPORTED, "%s needs H %% 128 == 0 and V %% 128 == 0 (H=%d V=%d)", dname, H, V);
    if (B <= 0 || T <= 0 || U1 <= 0 || V <= 0 || (need_h && H <= 0))
        return fail(RNNT_ERR_INVALID_ARG, "non-positive dimension B=%d T=%d U1=%d H=%d V=%d", B, T, U1, H, V);
    if (V % 4 != 0) return fail(RNNT_ERR_UNSUPPORTED, "V=%d must be a multiple of 4 (pad on the host side)", V);
    if (need_h && H % 4 != 0) return fail(RNNT_ERR_UNSUPPORTED, "H=%d must be a multiple of 4 (pad on the host side)", H);
    if (U1 > 1024) return fail(RNNT_ERR_UNSUPPORTED, "U1=%d exceeds 1024 lattice columns", U1);
    if ((long)T * U1 > 0x7fffffffL / 2) return fail(RNNT_ERR_UNSUPPORTED, "T*U1 too large");
    return RNNT_OK;
}

// FastEmit lambda / delay penalty delta of the *_reg entries: finite and >= 0, checked before anything else
int check_reg(float fastemit_lambda, float delay_penalty)
{
    if (!(fastemit_lambda >= 0.f && fastemit_lambda <= FLT_MAX))
        return fail(RNNT_ERR_INVALID_ARG, "fastemit_lambda=%g must be finite and >= 0", (double)fastemit_lambda);
    if (!(delay_penalty >= 0.f && delay_penalty <= FLT_MAX))
        return fail(RNNT_ERR_INVALID_ARG, "delay_penalty=%g must be finite and >= 0", (double)delay_penalty);
    return RNNT_OK;
}

// the alignment restriction of the *_restrict entries: a frames pointer and two buffers >= 0
int check_restrict(const int32_t *restrict_frames, int restrict_left, int restrict_right)
{
    if (!restrict_frames) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument (restrict_frames)");
    if (restrict_left < 0 || restrict_right < 0)
        return fail(RNNT_ERR_INVALID_ARG, "restrict_left=%d and restrict_right=%d must be >= 0", restrict_left, restrict_right);
    return RNNT_OK;
}

int dw_splits(int B, int T, int H, int V, int dtype)
{
    const long tiles = dtype == RNNT_DTYPE_F32 ? dw_tiles(H, V) : dtype == RNNT_DTYPE_F32_F16X2 ? x2_dw_tiles(H, V) : (long)((V + 255) / 256) * ((H + 255) / 256);
    long s = 256 / tiles;
    if (s < 1) s = 1;
    if (s > (long)B * T) s = (long)B * T;
    return (int)s;
}

// forward row tiles of 128; the dW DMA rings over-read up to DW_ROWS_PAST (zero) rows past rows_pad
long bf16_rows_alloc(size_t rows_pad) { return (long)((rows_pad + DW_ROWS_PAST + 127) / 128 * 128); }

void layout(int B, int T, int U1, int H, int V, int dtype, rnnt_engine_ws_layout *L)
{
    const size_t D = (size_t)T + U1 - 1;
    const size_t cells = (size_t)B * T * U1;
    const bool bf = dtype == RNNT_DTYPE_BF16, x2 = dtype == RNNT_DTYPE_F32_F16X2, x3 = dtype == RNNT_DTYPE_F32_BF16X3 || x2;
    // (x3: the split-operand routes — bf16x3, and f16x2 with two planes instead of three)
    // G / hidden rows are padded with >= 1 zero row up to a multiple of 16 (dW chunk size)
    // (bf16 / bf16x3 routes: multiple of 32 = one granule of their live-row table)
    const size_t rows_pad = (bf || x3) ? (cells + 1 + 31) / 32 * 32 : (cells + 1 + 15) / 16 * 16;
    L->rows_pad = rows_pad;
    L->D = (int)D;
    // dEnc slabs: one per u block; the fp32 route's fused dHidden kernel may use 8-wide blocks (the bf16x3
    // route can run its dHidden stage on that kernel: RNNT_VARIANT_X3_FP32_DH)
    L->n_ublk = bf ? (U1 + 15) / 16 : x3 ? (U1 + 7) / 8 : (U1 + dhidden_gen_bu(T, U1) - 1) / dhidden_gen_bu(T, U1);
    L->n_ttile = (T + 3) / 4;  // dPred slabs: at most one per 4 t rows (the persistent kernel's 16-wide items)
    L->n_split = dw_splits(B, T, H, V, dtype);
    L->g_lo = 0; L->aux = 0; L->aux_bytes = 0; L->x2_live = 0;
    size_t o = 0;
    if (bf) {
        const size_t ra = (size_t)bf16_rows_alloc(rows_pad);
        L->logits = o;   o += align_up(ra * V * 2);  // fp16
        L->hidden = o;   o += align_up(ra * H * 2);
    } else if (x3) {
        const size_t ra = (size_t)bf16_rows_alloc(rows_pad);
        L->logits = o;   o += align_up(ra * V * 4);      // fp32 logits; G hi | mid planes in place
        L->hidden = o;   o += align_up((x2 ? 2 : 3) * ra * H * 2);  // three bf16 planes (f16x2: two fp16 planes)
        if (!x2) { L->g_lo = o; o += align_up(ra * V * 2); }      // lo plane of G (f16x2: none — g_lo stays 0)
    } else {
        L->logits = o;   o += align_up((rows_pad + 16) * V * 4);
        L->hidden = o;   o += align_up((rows_pad + 16) * H * 4);
    }
    LatticeArgs w{};
    carve_loss_ws((void *)o, B, T, U1, w);  // the loss arrays: the standalone entries' carve, without its error word
    L->denom_s = (size_t)w.denom_s; L->lpb_s = (size_t)w.lpb_s; L->lpe_s = (size_t)w.lpe_s;
    L->alpha_s = (size_t)w.alpha_s; L->beta_s = (size_t)w.beta_s; L->coef = (size_t)w.coef; o = (size_t)w.err;
    L->wpack = o;
    if (bf) o += align_up(bf16_wpack_fwd_bytes(H, V)) + align_up(bf16_wpack_dh_bytes(H, V));
    else if (x2) o += align_up(x2_wpack_fwd_bytes(H, V)) + align_up(x2_wpack_dh_bytes(H, V));
    else if (x3) o += align_up(x3_wpack_fwd_bytes(H, V)) + align_up(x3_wpack_dh_bytes(H, V));
    else o += align_up(wpack_floats(H, V) * 4);
    L->enc_copy = o; o += align_up((size_t)B * T * H * 4);
    L->ep = 0;
    if (x2) { L->ep = o; o += align_up(x2_ep_bytes(B, T, U1, H)); }  // exp(2 enc) | exp(2 pred), k-step major (k_x2_make_ep)
    L->slab_enc = o; o += align_up((size_t)L->n_ublk * B * T * H * 4);
    L->slab_pred = o; o += align_up((size_t)L->n_ttile * B * U1 * H * 4);
    L->slab_w = o;   o += align_up((size_t)L->n_split * V * H * 4);
    L->slab_b = o;   o += align_up((size_t)L->n_split * V * 4);
    // the control block + the dW live-row table (bf16 routes) / live-granule list (fp32 route), whichever is larger, + the progress words
    const size_t tab = ControlBlock::dw_table_bytes(B), lst = (bf || x3) ? 0 : align_up(dw_list_bytes(B, T, U1, 16));
    L->counters = o; o += sizeof(ControlBlock) + (tab > lst ? tab : lst) + ((bf || x2) ? align_up((size_t)L->n_split * 64) : 0);
    if (x2) { L->x2_live = o; o += align_up(x2_live_bytes(B, T, U1, (long)rows_pad)); }  // counts, tile flags and list, k-step and group bitmaps and lists (launch_x2_live)
    L->total = o;
    if (x3) {  // fp32 hidden + fp32 W pack of the stages that can run on the fp32 route's kernels (RNNT_VARIANT_X3_FP32_*):
        // BEHIND `total` — only a call that asks for such a variant needs a workspace of total + aux_bytes
        L->aux = o; L->aux_bytes = align_up((rows_pad + 16) * H * 4) + align_up(wpack_floats(H, V) * 4);
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_fill32(unsigned *__restrict__ p, unsigned value, size_t n_words, int vec)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {  // 16-byte aligned, whole uint4s
        if (i < n_words / 4) ((u32x4 *)p)[i] = u32x4{value, value, value, value};
    } else if (i < n_words) {
        p[i] = value;
    }
}

__global__ __launch_bounds__(256) void k_copy32(unsigned *__restrict__ d, const unsigned *__restrict__ s, size_t n_words, int vec)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (vec) {
        if (i < n_words / 4) ((u32x4 *)d)[i] = ((const u32x4 *)s)[i];
    } else if (i < n_words) {
        d[i] = s[i];
    }
}

void launch_fill32(void *p, unsigned value, size_t bytes, hipStream_t st)
{
    const size_t n = bytes / 4;
    if (!n) return;
    const int vec = ((uintptr_t)p % 16 == 0) && (n % 4 == 0);
    const size_t thr = vec ? n / 4 : n;
    hipLaunchKernelGGL(k_fill32, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, st, (unsigned *)p, value, n, vec);
}

void launch_copy_bytes(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    const size_t n = bytes / 4;
    if (!n) return;
    const int vec = ((uintptr_t)dst % 16 == 0) && ((uintptr_t)src % 16 == 0) && (n % 4 == 0);
    const size_t thr = vec ? n / 4 : n;
    hipLaunchKernelGGL(k_copy32, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, st, (unsigned *)dst, (const unsigned *)src, n, vec);
}

namespace {

int launch_status(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(RNNT_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return RNNT_OK;
}

// Resolve enc into an h-contiguous, 16-byte friendly view (copying into the workspace when
// the caller's strides do not allow 16-byte row loads, e.g. the (B,C,T)->(B,T,C) permuted
// view of reference rnnt/model.py:28).
void resolve_enc(const void *enc, const int64_t s[3], int B, int T, int H, float *copy_buf,
                 hipStream_t st, const float **out, long *sb, long *st_)
{
    const bool direct = s[2] == 1 && (s[1] % 4) == 0 && (s[0] % 4) == 0 && aligned16(enc);
    if (direct) {
        *out = (const float *)enc; *sb = s[0]; *st_ = s[1];
    } else {
        launch_copy_enc((const float *)enc, s[0], s[1], s[2], copy_buf, B, T, H, st);
        *out = copy_buf; *sb = (long)T * H; *st_ = H;
    }
}

enum { ST_PROD = 1, ST_FWD = 2, ST_LATTICE = 4, ST_COEF = 8, ST_DH = 16, ST_DH_RED = 32, ST_DW = 64,
       ST_DW_RED = 128, ST_ALL = 255 };
// bits of the diagnostic word (-DRNNT_ABLATE builds) that are HOST-side experiments of the fp32 route
enum { ABLATE_NO_HIDDEN = 8, ABLATE_SEPARATE_G = 32, ABLATE_SEPARATE_HIDDEN = 64, ABLATE_FWD_LDS_RING = 128, ABLATE_FWD_ONE_WG = 256 };

// what the lattice and coefficient stages read (loss_stages), the fused routes' and the standalone loss entry's: the stages' argument block
// (carve_loss_ws, then the call's inputs and options: loss_call) and which of them run, where
struct LossCall : LatticeArgs { int stages /* ST_* mask */; hipStream_t st; };
void loss_call(LossCall &c, void *arrays, const int32_t *targets, const int32_t *logit_lens, const int32_t *target_lens, float *costs, int B,
               int T, int U1, int stages, float grad_scale, float fastemit, float delay, hipStream_t st, const int32_t *restrict_frames,
               int restrict_left, int restrict_right)
{
    carve_loss_ws(arrays, B, T, U1, c);
    c.targets = targets; c.logit_lens = logit_lens; c.target_lens = target_lens; c.costs = costs; c.stages = stages; c.st = st;
    c.grad_scale = grad_scale; c.fastemit = fastemit; c.delay = delay;
    c.restrict_frames = restrict_frames; c.restrict_left = restrict_left; c.restrict_right = restrict_right;
}

// One fused call after validation: what the routes and the argument fillers read.  The standalone joint entries fill
// what their launches read: fwd_args takes dims, the enc view, pred, bias and logits (cb may be null, the loss arrays too); bwd_args also ws, L, cb.
struct FusedCall : LossCall {
    int H, n_cu;  // (V and blank: LatticeArgs')
    const float *enc, *pred, *W, *bias; long enc_sb, enc_st;  // enc: the resolved view (resolve_enc)
    float *grad_enc, *grad_pred, *grad_W, *grad_bias;
    rnnt_engine_ws_layout L;
    char *ws; ControlBlock *cb; float *joint_logits;
    bool separate_g, separate_hidden, fwd_lds_ring, fwd_one_wg_per_tile, no_hidden;  // the fp32 route's forms: RNNT_VARIANT_*, ABLATE_*
    bool x3_fp32_fwd, x3_fp32_dh;  // split routes: the stage runs on the fp32 route's kernels (RNNT_VARIANT_X3_FP32_*, or a shape not covered)
    bool x2_no_flush;              // f16x2: no cell is flushed (RNNT_VARIANT_X2_NO_FLUSH_SKIP, or a regularised loss)
    int ablate; unsigned long long *debug;  // diagnostic builds: rnnt_engine_set_flags / rnnt_engine_set_debug, else 0 / NULL
};
float *f32_at(const FusedCall &c, size_t offset) { return (float *)(c.ws + offset); }

// ---- the argument structs, each filled in one place (what a filler does not set is zero / NULL)
JointFwdArgs fwd_args(const FusedCall &c, const float *wpack, const float *hidden, int make_hidden)
{
    JointFwdArgs f{};
    f.enc = c.enc; f.enc_sb = c.enc_sb; f.enc_st = c.enc_st; f.pred = c.pred; f.logit_lens = c.logit_lens; f.target_lens = c.target_lens;
    f.B = c.B; f.T = c.T; f.U1 = c.U1; f.H = c.H; f.V = c.V; f.blank = c.blank; f.ablate = c.ablate; f.debug = c.debug;
    f.wpack = wpack; f.hidden = hidden; f.make_hidden = make_hidden; f.bias = c.bias; f.targets = c.targets; f.logits = c.joint_logits;
    f.denom_s = c.denom_s; f.lpb_s = c.lpb_s; f.lpe_s = c.lpe_s; f.D = c.L.D; f.counter = c.cb ? c.cb->fwd_tile : nullptr; f.n_cu = c.n_cu;
    return f;
}

JointBwdArgs bwd_args(const FusedCall &c)
{
    JointBwdArgs g{};
    g.enc = c.enc; g.enc_sb = c.enc_sb; g.enc_st = c.enc_st; g.pred = c.pred; g.logit_lens = c.logit_lens; g.target_lens = c.target_lens;
    g.B = c.B; g.T = c.T; g.U1 = c.U1; g.H = c.H; g.V = c.V; g.blank = c.blank; g.ablate = c.ablate; g.debug = c.debug;
    g.W = c.W; g.logits = c.joint_logits; g.coef = c.coef; g.hidden = f32_at(c, c.L.hidden); g.rows_pad = (long)c.L.rows_pad;
    g.slab_enc = f32_at(c, c.L.slab_enc); g.slab_pred = f32_at(c, c.L.slab_pred);
    g.slab_w = f32_at(c, c.L.slab_w); g.slab_b = f32_at(c, c.L.slab_b);
    g.grad_enc = c.grad_enc; g.grad_pred = c.grad_pred; g.grad_W = c.grad_W; g.grad_bias = c.grad_bias;
    g.n_ublk = c.L.n_ublk; g.n_ttile = c.L.n_ttile; g.n_split = c.L.n_split;
    g.counter = c.cb->queue; g.dw_tab = c.cb->dw_tab(); g.n_cu = c.n_cu;
    g.gen_bu = dhidden_gen_bu(c.T, c.U1);  // u width of the fp32 route's dHidden tiles (the other routes: 16)
    return g;
}

template <class Args> Args split_args(const FusedCall &c, size_t wpack_fwd_bytes)  // what Bf16Args and X3Args share; the dHidden pack lies behind the forward's
{
    Args h{};
    h.enc = c.enc; h.enc_sb = c.enc_sb; h.enc_st = c.enc_st; h.pred = c.pred; h.logit_lens = c.logit_lens; h.target_lens = c.target_lens;
    h.B = c.B; h.T = c.T; h.U1 = c.U1; h.H = c.H; h.V = c.V; h.blank = c.blank; h.ablate = c.ablate; h.debug = c.debug;
    h.W = c.W; h.bias = c.bias; h.targets = c.targets; h.coef = c.coef; h.hidden = (unsigned short *)(c.ws + c.L.hidden);
    h.denom_s = c.denom_s; h.lpb_s = c.lpb_s; h.lpe_s = c.lpe_s; h.D = c.L.D;
    h.slab_enc = f32_at(c, c.L.slab_enc); h.slab_pred = f32_at(c, c.L.slab_pred);
    h.slab_w = f32_at(c, c.L.slab_w); h.slab_b = f32_at(c, c.L.slab_b);
    h.rows_pad = (long)c.L.rows_pad; h.rows_alloc = bf16_rows_alloc(c.L.rows_pad);
    h.n_ublk = c.L.n_ublk; h.n_split = c.L.n_split; h.dw_tab = c.cb->dw_tab();
    h.wpack_fwd = c.ws + c.L.wpack; h.wpack_dh = c.ws + c.L.wpack + align_up(wpack_fwd_bytes);
    return h;
}

Bf16Args bf16_args(const FusedCall &c)
{
    Bf16Args h = split_args<Bf16Args>(c, bf16_wpack_fwd_bytes(c.H, c.V));
    h.logits = (unsigned short *)c.joint_logits; h.dw_prog = c.cb->dw_prog(c.B);
    return h;
}

// f16x2 operand scales: |G| <= (1 + fastemit) grad_scale <= 2^e -> g_scale = 2^(13 - e); hidden: 2^14 (x2.hip).
// (FastEmit adds lambda E (p_k - [k = y]) with E <= 1 to a cell's G: DESIGN.md §4k; the bound of the stand-in dHidden's split of G is the
// same g_scale.)  flush_log2 / flush_lin: the flush rule's threshold (x2.hip), log2 of 2^-26 / g_scale and that value itself.
struct OperandScales { float g_scale, dw_rescale, db_rescale; double flush_log2; float flush_lin; };
OperandScales operand_scales(float grad_scale, float fastemit)
{
    OperandScales s; int e = 0;
    (void)frexpf(grad_scale * (1.0f + fastemit), &e);
    const int k = 13 - e < -100 ? -100 : (13 - e > 100 ? 100 : 13 - e);
    s.g_scale = ldexpf(1.0f, k); s.flush_log2 = (double)(-26 - k); s.flush_lin = ldexpf(1.0f, -26 - k);
    s.dw_rescale = 1.0f / (s.g_scale * 16384.0f); s.db_rescale = 1.0f / s.g_scale;
    return s;
}

X3Args x3_args(const FusedCall &c, size_t wpack_fwd_bytes, const OperandScales &s)  // both split routes (f16x2 adds to it: route_f16x2)
{
    X3Args h = split_args<X3Args>(c, wpack_fwd_bytes);
    h.g_scale = s.g_scale; h.dw_rescale = s.dw_rescale; h.db_rescale = s.db_rescale; h.scales = c.cb->x2_scales;
    h.ep_enc = f32_at(c, c.L.ep); h.ep_pred = h.ep_enc + (size_t)c.B * c.T * c.H; h.ep_flag = c.cb->ep_flag;
    h.logits = c.joint_logits; h.g_lo = (unsigned short *)(c.ws + c.L.g_lo); h.n_ublk16 = (c.U1 + 15) / 16;
    h.plane_stride = h.rows_alloc * (long)c.H; h.counter = c.cb->fwd_tile; h.n_cu = c.n_cu;
    return h;
}

// lattice sweep and coefficients (every route): the pass over lp_emit — the delay penalty and the alignment restriction
// (§4n) — before the sweep, the penalty's cost shift off after it, then the coefficients; zero options launch exactly the plain loss's
// kernels.  flush: the f16x2 route's thresholds (lattice.hip k_coef), or null: no flush rule.  Which sweep and which coefficient kernel run is
// the launchers' business.
void loss_stages(const LossCall &c, const OperandScales *flush = nullptr)
{
    LatticeArgs a = c;
    if (flush) { a.flush = true; a.flush_log2 = flush->flush_log2; a.flush_lin = flush->flush_lin; }
    if (c.stages & ST_LATTICE) {
        if (a.restrict_frames || a.delay > 0.f) launch_lp_emit(a, c.st);
        launch_lattice(a, c.st);
        if (a.delay > 0.f) launch_delay_cost(a, c.st);
    }
    if (c.stages & ST_COEF) launch_coef(a, c.st);
}

void zero_unwritten_hidden(const FusedCall &c, float *hidden)  // what a forward filling fp32 hidden leaves: padding rows, dead cells
{
    const size_t cells = (size_t)c.B * c.T * c.U1;
    launch_fill32(hidden + cells * c.H, 0u, (c.L.rows_pad + 16 - cells) * c.H * 4, c.st);
    launch_zero_dead_hidden(hidden, c.logit_lens, c.target_lens, c.B, c.T, c.U1, c.H, c.st);
}

// columns the fp32 route's tile kernel (k_dhidden_gen) takes at this shape: whole groups of 512, 8-row dPred slabs; 0: the persistent k_dhidden on every column
int tile_kernel_cols(const FusedCall &c) { return dhidden_gen_ok(c.H, c.V, c.U1) ? 512 * dhidden_gen_groups(c.H) : 0; }

// The split routes' stand-in stages: the fp32 route's kernel in place of a split one, on the fp32 hidden and W pack in `aux`
float *aux_hidden(const FusedCall &c) { return f32_at(c, c.L.aux); }
typedef void (*x3_launcher)(const X3Args &, hipStream_t);

void standin_forward(const FusedCall &c, const X3Args &h, x3_launcher make_hidden)
{
    float *wpack = (float *)(c.ws + c.L.aux + align_up((c.L.rows_pad + 16) * (size_t)c.H * 4));
    if (c.stages & ST_PROD) { zero_unwritten_hidden(c, aux_hidden(c)); launch_pack_w_fwd(c.W, wpack, c.H, c.V, c.st); }
    if (c.stages & ST_FWD) {
        JointFwdArgs f = fwd_args(c, wpack, aux_hidden(c), 1);
        f.ablate = 0; f.debug = nullptr;  // a stand-in takes no part in a diagnostic build's experiments
        launch_joint_fwd(f, c.st); make_hidden(h, c.st);  // then the planes the backward reads
    }
}

void standin_dhidden(const FusedCall &c, const JointBwdArgs &g, const X3Args &h, x3_launcher split_g)
{
    const bool tile = g.pred_split_col > 0;
    if (!tile) launch_make_g(g, c.st);
    launch_dhidden(g, tile, c.st);  // leaves fp32 G in place of the logits
    split_g(h, c.st);               // -> the route's planes in place (bf16x3: lo beside)
}

int route_fp32(const FusedCall &c)
{
    JointBwdArgs g = bwd_args(c);
    // G inside the dHidden GEMM unless the shape needs the separate pass (k_make_g, then the persistent k_dhidden on every column).
    // RNNT_VARIANT_SEPARATE_G runs k_make_g at a shape the tile kernel takes: the tile kernel then READS G in its first column group too
    // (GEN = false) and forms every sum in the default order — bit-identical results, as the header says
    const bool tile = (g.pred_split_col = tile_kernel_cols(c)) > 0, fuse_g = tile && !c.separate_g;
    g.g_ready = tile && !fuse_g;
    // hidden (A operand of all three GEMMs) is produced by the forward kernel for its own tile unless the separate k_make_hidden pass is asked for
    const bool fuse_hid = !c.separate_hidden && !c.no_hidden;
    float *wpack = (float *)(c.ws + c.L.wpack);
    if (c.stages & ST_PROD) {
        if (fuse_hid) zero_unwritten_hidden(c, g.hidden);
        else launch_make_hidden(g, c.st);
        launch_pack_w_fwd(c.W, wpack, c.H, c.V, c.st);
    }
    if (c.stages & ST_FWD)
        launch_joint_fwd(fwd_args(c, wpack, c.no_hidden ? nullptr : g.hidden, fuse_hid ? 1 : 0), c.st, c.fwd_lds_ring, c.fwd_one_wg_per_tile);
    loss_stages(c);
    if ((c.stages & ST_COEF) && !fuse_g) launch_make_g(g, c.st);  // logits -> G in place
    if (c.stages & ST_DH) launch_dhidden(g, tile, c.st);
    if (c.stages & ST_DH_RED) launch_dhidden_reduce(g, c.st);
    if (c.stages & ST_DW) launch_dw(g, c.st);
    if (c.stages & ST_DW_RED) launch_dw_reduce(g, c.st);
    return launch_status("rnnt_engine fused pipeline");
}

int route_bf16(const FusedCall &c)
{
    const Bf16Args h = bf16_args(c);
    JointBwdArgs g = bwd_args(c); g.gen_bu = 16; g.pred_split_col = c.H;  // the reductions: 16-wide u tiles, every dPred slab 8 t-rows high
    if (c.stages & ST_PROD) launch_bf16_producers(h, c.st);
    if (c.stages & ST_FWD) launch_joint_fwd_bf16(h, c.st);  // softmax statistics in its epilogue
    loss_stages(c);
    if (c.stages & ST_DH) launch_dhidden_bf16(h, c.st);
    if (c.stages & ST_DH_RED) launch_dhidden_reduce(g, c.st);
    if (c.stages & ST_DW) launch_dw_bf16(h, c.st);
    if (c.stages & ST_DW_RED) launch_dw_reduce(g, c.st);
    return launch_status("rnnt_engine fused pipeline (bf16)");
}

// the fp32 kernels' view of a split route's call: the dHidden reductions', the stand-in dHidden's
JointBwdArgs split_bwd_args(const FusedCall &c)
{
    JointBwdArgs g = bwd_args(c); g.hidden = aux_hidden(c);
    if (c.x3_fp32_dh) g.pred_split_col = tile_kernel_cols(c);
    else { g.gen_bu = 16; g.pred_split_col = c.H; }  // x3 / x2 tiles: 8 t x 16 u, every dPred slab 8 t rows high
    return g;
}

// fp32-accurate route on the bf16 matrix pipes (x3.hip)
int route_bf16x3(const FusedCall &c)
{
    const X3Args h = x3_args(c, x3_wpack_fwd_bytes(c.H, c.V), operand_scales(c.grad_scale, c.fastemit));
    JointBwdArgs g = split_bwd_args(c);
    if (c.stages & ST_PROD) { launch_x3_zero_padding(h, 1, c.st); launch_x3_pack_w(h, c.st); }
    if (c.x3_fp32_fwd) standin_forward(c, h, launch_x3_make_hidden);
    else if (c.stages & ST_FWD) launch_joint_fwd_x3(h, c.st);
    loss_stages(c);
    if (c.stages & ST_DH) {
        launch_x3_zero_padding(h, 2, c.st);
        if (c.x3_fp32_dh) standin_dhidden(c, g, h, launch_x3_split_g);  // -> hi | mid in place, lo beside
        else launch_dhidden_x3(h, c.st);
    }
    if (c.stages & ST_DH_RED) launch_dhidden_reduce(g, c.st);
    if (c.stages & ST_DW) launch_dw_x3(h, c.st);
    if (c.stages & ST_DW_RED) launch_dw_reduce(g, c.st);
    return launch_status("rnnt_engine fused pipeline (bf16x3)");
}

// the same stages on two fp16 planes and three products (x2.hip), with the flush rule: dHidden / dW walk the live tiles / groups only
int route_f16x2(const FusedCall &c)
{
    OperandScales s = operand_scales(c.grad_scale, c.fastemit);
    X3Args h = x3_args(c, x2_wpack_fwd_bytes(c.H, c.V), s);
    h.dw_prog = c.cb->dw_prog(c.B); h.dw_ksteps = x2_dw_walks_ksteps(c.H, c.V) ? 1 : 0;
    x2_live_carve(c.ws + c.L.x2_live, c.B, c.T, c.U1, (long)c.L.rows_pad, h);
    JointBwdArgs g = split_bwd_args(c);
    // k_dhidden_x2 runs the live tiles only and no dead tile writes a slab: the reductions skip by the same flags
    if (!c.x3_fp32_dh) { g.tile_flag = h.tile_live; g.flag_ntt = (c.T + 7) / 8; g.flag_nub = h.n_ublk16; }
    // The threshold; -inf flags nothing.  The fp32 kernels standing in for dHidden multiply G in fp32, where a flushed cell's G is small but not
    // zero: no flush, no tile skipping there (k_split_g writes every row, so the dW list walk still applies)
    if (c.x2_no_flush || c.x3_fp32_dh) { s.flush_log2 = -HUGE_VAL; s.flush_lin = 0.f; }
    if (c.stages & ST_PROD) { launch_x2_zero_padding(h, 1, c.st); launch_x2_pack_w(h, c.cb->x2_scales, c.st); launch_x2_make_ep(h, c.st); }
    if (c.x3_fp32_fwd) standin_forward(c, h, launch_x2_make_hidden);
    else if (c.stages & ST_FWD) launch_joint_fwd_x2(h, c.st);
    loss_stages(c, &s);
    if (c.stages & ST_COEF) launch_x2_live(h, c.st);  // tile flags, k-step and group bitmaps / lists, counts: from the coefficients
    if (c.stages & ST_DH) {
        launch_x2_zero_padding(h, 2, c.st);
        // (dead rows: those of dead tiles inside live groups — k_dw_x2m: k-steps —, zeros for dW; disjoint from the live tiles' rows)
        if (c.x3_fp32_dh) standin_dhidden(c, g, h, launch_x2_split_g);
        else { launch_x2_dead_rows(h, c.st); launch_dhidden_x2(h, c.st); }
    }
    if (c.stages & ST_DH_RED) launch_dhidden_reduce(g, c.st);
    if (c.stages & ST_DW) launch_dw_x2(h, c.st);
    if (c.stages & ST_DW_RED) launch_dw_reduce_x2(h, c.grad_W, c.grad_bias, c.st);  // one rounding: dW does not follow where the splits cut the live list
    return launch_status("rnnt_engine fused pipeline (f16x2)");
}

// Every fused entry: validation (everything that can fail does so here, before anything is launched), the call context, the route.
int run_fused(int stages, int variant, const void *enc, const int64_t enc_strides[3], const void *pred,
              const void *W, const void *bias, const int32_t *targets, const int32_t *logit_lens,
              const int32_t *target_lens, int B, int T, int U1, int H, int V, int blank,
              float clamp, float grad_scale, float fastemit, float delay, int dtype, float *costs,
              void *grad_enc, void *grad_pred, void *grad_W, void *grad_bias, void *workspace,
              size_t ws_bytes, void *stream, const int32_t *restrict_frames = nullptr, int restrict_left = 0,
              int restrict_right = 0)
{
    if (int rc = check_dims(B, T, U1, H, V, dtype, true)) return rc;
    if (!enc || !enc_strides || !pred || !W || !bias || !targets || !logit_lens || !target_lens ||
        !costs || !workspace)
        return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    const bool backward = (stages & (ST_DH | ST_DH_RED | ST_DW | ST_DW_RED)) != 0;
    if (backward && (!grad_enc || !grad_pred || !grad_W || !grad_bias))
        return fail(RNNT_ERR_INVALID_ARG, "null gradient pointer");
    if (blank < 0 || blank >= V) return fail(RNNT_ERR_INVALID_ARG, "blank=%d outside [0,%d)", blank, V);
    if (clamp > 0.f) return fail(RNNT_ERR_UNSUPPORTED, "clamp>0 is only supported by rnnt_engine_loss_fwd_bwd");
    if (!(grad_scale > 0.f)) return fail(RNNT_ERR_INVALID_ARG, "grad_scale must be > 0");
    if (!aligned16(pred) || !aligned16(W) || !aligned16(bias) || !aligned16(grad_enc) ||
        !aligned16(grad_pred) || !aligned16(grad_W) || !aligned16(grad_bias) ||
        ((uintptr_t)workspace & 255))
        return fail(RNNT_ERR_INVALID_ARG, "pointers must be 16-byte aligned (workspace 256)");
    // bits 14 and up once named kernels measured equal to (or slower than) the shipped ones; those kernels are gone and the bits stay
    // reserved: refused here, before anything is launched, instead of silently running something else
    if (variant & RNNT_VARIANT_LAB_MASK)
        return fail(RNNT_ERR_UNSUPPORTED, "variant bits 0x%x are reserved: no kernel of librnnt_engine.so answers to them",
                    variant & RNNT_VARIANT_LAB_MASK);
    FusedCall c{};
    layout(B, T, U1, H, V, dtype, &c.L);
    if (ws_bytes < c.L.total)
        return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, c.L.total);
    c.ablate = g_flags; c.debug = g_debug;
    const int xp = dtype == RNNT_DTYPE_F32 ? c.ablate : 0;  // the fp32 route's host-side experiments (no kernel of that route reads these bits)
    c.separate_g = (variant & RNNT_VARIANT_SEPARATE_G) != 0 || (xp & ABLATE_SEPARATE_G) != 0;
    c.separate_hidden = (variant & RNNT_VARIANT_SEPARATE_HIDDEN) != 0 || (xp & ABLATE_SEPARATE_HIDDEN) != 0;
    c.fwd_lds_ring = (variant & RNNT_VARIANT_FWD_LDS_RING) != 0 || (xp & ABLATE_FWD_LDS_RING) != 0;
    c.fwd_one_wg_per_tile = (variant & RNNT_VARIANT_FWD_ONE_WG_PER_TILE) != 0 || (xp & ABLATE_FWD_ONE_WG) != 0;
    c.no_hidden = (xp & ABLATE_NO_HIDDEN) != 0;
    c.x2_no_flush = (variant & RNNT_VARIANT_X2_NO_FLUSH_SKIP) != 0 || fastemit > 0.f || delay > 0.f;
    if (dtype == RNNT_DTYPE_F32_BF16X3 || dtype == RNNT_DTYPE_F32_F16X2) {
        const bool x2 = dtype == RNNT_DTYPE_F32_F16X2;
        c.x3_fp32_dh = (variant & RNNT_VARIANT_X3_FP32_DH) != 0 || !(x2 ? x2_dhidden_ok(U1, H, V) : x3_dhidden_ok(U1, H, V));
        c.x3_fp32_fwd = (variant & RNNT_VARIANT_X3_FP32_FWD) != 0 || !split_fwd_ok(U1, H, V) || c.x3_fp32_dh;  // fp32 dHidden reads fp32 hidden
        if (c.x3_fp32_fwd && ws_bytes < c.L.total + c.L.aux_bytes)
            return fail(RNNT_ERR_WORKSPACE, "workspace %zu < %zu bytes: a stage on the fp32 route's kernels (RNNT_VARIANT_X3_FP32_*, or a "
                        "shape k_joint_fwd_x3 / k_dhidden_x3 do not cover) needs total + aux_bytes of rnnt_engine_workspace_layout",
                        ws_bytes, c.L.total + c.L.aux_bytes);
    }
    c.H = H; c.V = V; c.blank = blank; c.pred = (const float *)pred; c.W = (const float *)W; c.bias = (const float *)bias;
    c.grad_enc = (float *)grad_enc; c.grad_pred = (float *)grad_pred; c.grad_W = (float *)grad_W; c.grad_bias = (float *)grad_bias;
    c.n_cu = device_cus(); c.ws = (char *)workspace; c.cb = (ControlBlock *)(c.ws + c.L.counters); c.joint_logits = f32_at(c, c.L.logits);
    loss_call(c, c.ws + c.L.denom_s, targets, logit_lens, target_lens, costs, B, T, U1, stages, grad_scale, fastemit, delay,
              (hipStream_t)stream, restrict_frames, restrict_left, restrict_right);  // (layout() places the arrays by the same carve)
    c.err = c.cb->lattice_err;
    resolve_enc(enc, enc_strides, B, T, H, f32_at(c, c.L.enc_copy), c.st, &c.enc, &c.enc_sb, &c.enc_st);
    if (dtype == RNNT_DTYPE_BF16) return route_bf16(c);
    if (dtype == RNNT_DTYPE_F32_BF16X3) return route_bf16x3(c);
    return dtype == RNNT_DTYPE_F32_F16X2 ? route_f16x2(c) : route_fp32(c);
}

}  // namespace

extern "C" {

int rnnt_engine_version(void) { return RNNT_ENGINE_VERSION; }

#if defined(RNNT_ABLATE) || defined(RNNT_STAMPS)
int rnnt_engine_set_flags(int flags) { int o = g_flags; g_flags = flags; return o; }
void rnnt_engine_set_debug(void *buf) { g_debug = (unsigned long long *)buf; }
#else  // shipped build: no process-wide state; the symbols stay so diagnostic tools link
int rnnt_engine_set_flags(int) { return 0; }
void rnnt_engine_set_debug(void *) {}
#endif

int rnnt_engine_debug_query(int what) { return fwd_occupancy(what); }

const char *rnnt_engine_last_error(void) { return g_err.c_str(); }

// ---- RCCL all-reduce of the flat gradient buffer.  No link-time dependency: the symbol
// comes from the RCCL already in the process (soname librccl.so.1: PyTorch-ROCm's copy when torch is
// loaded), so the communicator the caller made and the function called belong to the same library.
int rnnt_engine_allreduce(void *buf, size_t count, void *comm, void *stream)
{
    if (!buf || !comm) return fail(RNNT_ERR_INVALID_ARG, "null buffer / communicator");
    if (count == 0) return RNNT_OK;
    typedef int (*allreduce_fn)(const void *, void *, size_t, int, int, void *, hipStream_t);
    typedef const char *(*errstr_fn)(int);
    void *sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");
    void *lib = nullptr;
    if (!sym) {
        lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);  // the copy that is already loaded
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW);
        if (lib) sym = dlsym(lib, "ncclAllReduce");
    }
    if (!sym) return fail(RNNT_ERR_UNSUPPORTED, "RCCL (librccl.so.1: ncclAllReduce) not found in this process");
    const int ncclFloat32_ = 7, ncclSum_ = 0;  // rccl.h: ncclDataType_t / ncclRedOp_t
    const int rc = ((allreduce_fn)sym)(buf, buf, count, ncclFloat32_, ncclSum_, comm, (hipStream_t)stream);
    if (rc != 0) {
        void *es = lib ? dlsym(lib, "ncclGetErrorString") : dlsym(RTLD_DEFAULT, "ncclGetErrorString");
        return fail(RNNT_ERR_LAUNCH, "ncclAllReduce failed (%d): %s", rc, es ? ((errstr_fn)es)(rc) : "?");
    }
    return RNNT_OK;
}

int rnnt_engine_workspace_layout(int B, int T, int U1, int H, int V, int dtype,
                                 rnnt_engine_ws_layout *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null layout pointer");
    if (int rc = check_dims(B, T, U1, H, V, dtype, true)) return rc;
    layout(B, T, U1, H, V, dtype, out);
    return RNNT_OK;
}

int rnnt_engine_workspace_bytes(int B, int T, int U1, int H, int V, int dtype, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    rnnt_engine_ws_layout L;
    if (int rc = rnnt_engine_workspace_layout(B, T, U1, H, V, dtype, &L)) return rc;
    *out = L.total;
    return RNNT_OK;
}

int rnnt_engine_loss_workspace_bytes(int B, int T, int U1, int V, int dtype, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (int rc = check_dims(B, T, U1, 4, V, dtype, false)) return rc;
    LatticeArgs a{};
    *out = carve_loss_ws(nullptr, B, T, U1, a);
    return RNNT_OK;
}

int rnnt_engine_joint_fwd_workspace_bytes(int B, int T, int U1, int H, int V, int dtype,
                                          size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (int rc = check_dims(B, T, U1, H, V, dtype, true)) return rc;
    *out = align_up(wpack_floats(H, V) * 4) + align_up((size_t)B * T * H * 4);
    return RNNT_OK;
}

int rnnt_engine_joint_fwd(const void *enc, const int64_t enc_strides[3], const void *pred,
                          const void *W, const void *bias, int B, int T, int U1, int H, int V,
                          int dtype, void *logits, void *workspace, size_t ws_bytes, void *stream)
{
    if (int rc = check_dims(B, T, U1, H, V, dtype, true)) return rc;
    if (!enc || !enc_strides || !pred || !W || !bias || !logits || !workspace)
        return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    if (!aligned16(pred) || !aligned16(W) || !aligned16(bias) || !aligned16(logits) ||
        ((uintptr_t)workspace & 255))
        return fail(RNNT_ERR_INVALID_ARG, "pointers must be 16-byte aligned (workspace 256)");
    size_t need;
    rnnt_engine_joint_fwd_workspace_bytes(B, T, U1, H, V, dtype, &need);
    if (ws_bytes < need) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
    FusedCall c{};  // the plain joint: no loss arrays, no control block (one workgroup per tile); workspace: W pack | enc copy
    c.B = B; c.T = T; c.U1 = U1; c.H = H; c.V = V; c.blank = V - 1; c.L.D = T + U1 - 1;
    c.pred = (const float *)pred; c.W = (const float *)W; c.bias = (const float *)bias; c.joint_logits = (float *)logits;
    c.ablate = g_flags; c.debug = g_debug; c.st = (hipStream_t)stream;
    float *wpack = (float *)workspace, *enc_copy = (float *)((char *)workspace + align_up(wpack_floats(H, V) * 4));
    resolve_enc(enc, enc_strides, B, T, H, enc_copy, c.st, &c.enc, &c.enc_sb, &c.enc_st);
    launch_pack_w_fwd(c.W, wpack, H, V, c.st);
    launch_joint_fwd(fwd_args(c, wpack, nullptr, 0), c.st);
    return launch_status("rnnt_engine_joint_fwd");
}

int rnnt_engine_joint_bwd_workspace_bytes(int B, int T, int U1, int H, int V, int dtype, size_t *out)
{
    if (dtype != RNNT_DTYPE_F32) return fail(RNNT_ERR_UNSUPPORTED, "rnnt_engine_joint_bwd is fp32 only");
    return rnnt_engine_workspace_bytes(B, T, U1, H, V, dtype, out);
}

int rnnt_engine_joint_bwd(const void *enc, const int64_t enc_strides[3], const void *pred,
                          const void *W, const void *grad_logits, int B, int T, int U1, int H, int V,
                          int dtype, void *grad_enc, void *grad_pred, void *grad_W, void *grad_bias,
                          void *workspace, size_t ws_bytes, void *stream)
{
    if (dtype != RNNT_DTYPE_F32) return fail(RNNT_ERR_UNSUPPORTED, "rnnt_engine_joint_bwd is fp32 only");
    if (int rc = check_dims(B, T, U1, H, V, dtype, true)) return rc;
    if (!enc || !enc_strides || !pred || !W || !grad_logits || !grad_enc || !grad_pred || !grad_W ||
        !grad_bias || !workspace)
        return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    if (!aligned16(pred) || !aligned16(W) || !aligned16(grad_logits) || !aligned16(grad_enc) ||
        !aligned16(grad_pred) || !aligned16(grad_W) || !aligned16(grad_bias) || ((uintptr_t)workspace & 255))
        return fail(RNNT_ERR_INVALID_ARG, "pointers must be 16-byte aligned (workspace 256)");
    FusedCall c{};  // the fp32 route's workspace; no loss arrays (no coefficients), no diagnostics
    layout(B, T, U1, H, V, dtype, &c.L);
    if (ws_bytes < c.L.total) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, c.L.total);
    hipStream_t st = c.st = (hipStream_t)stream;
    c.ws = (char *)workspace; c.cb = (ControlBlock *)(c.ws + c.L.counters); c.joint_logits = f32_at(c, c.L.logits);  // G
    // every utterance at full length: the upstream gradient is dense (zero where the caller's loss
    // ignored a cell); the length arrays the kernels read live in the (unused) coefficient region
    int32_t *ll = (int32_t *)(c.ws + c.L.coef), *tl = ll + B;
    c.B = B; c.T = T; c.U1 = U1; c.H = H; c.V = V; c.blank = V - 1; c.n_cu = device_cus();
    c.pred = (const float *)pred; c.W = (const float *)W; c.logit_lens = ll; c.target_lens = tl;
    c.grad_enc = (float *)grad_enc; c.grad_pred = (float *)grad_pred; c.grad_W = (float *)grad_W; c.grad_bias = (float *)grad_bias;
    resolve_enc(enc, enc_strides, B, T, H, f32_at(c, c.L.enc_copy), st, &c.enc, &c.enc_sb, &c.enc_st);
    launch_fill32(ll, (unsigned)T, (size_t)B * 4, st);
    launch_fill32(tl, (unsigned)(U1 - 1), (size_t)B * 4, st);
    // G with the zero padding rows the dW GEMM walks past the last cell
    const size_t cells = (size_t)B * T * U1;
    launch_copy_bytes(c.joint_logits, grad_logits, cells * V * 4, st);
    launch_fill32(c.joint_logits + cells * V, 0u, (c.L.rows_pad + 16 - cells) * V * 4, st);
    const JointBwdArgs g = bwd_args(c);
    launch_make_hidden(g, st);
    launch_dhidden(g, false, st);  // G is given: the persistent kernel on every column
    launch_dhidden_reduce(g, st);
    launch_dw(g, st);
    launch_dw_reduce(g, st);
    return launch_status("rnnt_engine_joint_bwd");
}

int rnnt_engine_greedy_scan_workspace_bytes(int nframes, int H, int V, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (nframes < 1 || nframes > 128) return fail(RNNT_ERR_INVALID_ARG, "nframes=%d outside [1,128]", nframes);
    if (int rc = check_dims(1, nframes, 1, H, V, RNNT_DTYPE_F32, true)) return rc;
    if (H % 8 != 0) return fail(RNNT_ERR_UNSUPPORTED, "greedy scan needs H %% 8 == 0 (H=%d)", H);
    *out = align_up((size_t)nframes * H * 4) + align_up((size_t)nframes * V * 4);
    return RNNT_OK;
}

int rnnt_engine_greedy_scan(const void *enc, int64_t enc_stride_t, int64_t enc_stride_h, const void *pred,
                            const void *W, const void *bias, int t0, int nframes, int H, int V, int blank,
                            int32_t *out, void *workspace, size_t ws_bytes, void *stream)
{
    size_t need;
    if (int rc = rnnt_engine_greedy_scan_workspace_bytes(nframes, H, V, &need)) return rc;
    if (!enc || !pred || !W || !bias || !out || !workspace) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    if (t0 < 0) return fail(RNNT_ERR_INVALID_ARG, "t0=%d is negative", t0);
    if (blank < 0 || blank >= V) return fail(RNNT_ERR_INVALID_ARG, "blank=%d outside [0,%d)", blank, V);
    if (!aligned16(pred) || !aligned16(W) || !aligned16(bias) || ((uintptr_t)workspace & 255))
        return fail(RNNT_ERR_INVALID_ARG, "pointers must be 16-byte aligned (workspace 256)");
    if (ws_bytes < need) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    float *enc_copy = (float *)ws;
    float *logits = (float *)(ws + align_up((size_t)nframes * H * 4));
    const int64_t strides[3] = {0, enc_stride_t, enc_stride_h};
    const float *encp; long esb, est;
    resolve_enc((const float *)enc + (int64_t)t0 * enc_stride_t, strides, 1, nframes, H, enc_copy, st, &encp, &esb, &est);
    launch_scan_logits(encp, est, (const float *)pred, (const float *)W, (const float *)bias, logits, nframes, H, V, st);
    launch_argmax_scan(logits, nframes, V, blank, t0, out, st);
    return launch_status("rnnt_engine_greedy_scan");
}

int rnnt_engine_greedy_decode_workspace_bytes(int H, int V, int E, int O, int scan_frames, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (scan_frames < 1 || scan_frames > 128) return fail(RNNT_ERR_INVALID_ARG, "scan_frames=%d outside [1,128]", scan_frames);
    if (int rc = check_dims(1, scan_frames, 1, H, V, RNNT_DTYPE_F32, true)) return rc;
    if (H % 8 != 0) return fail(RNNT_ERR_UNSUPPORTED, "greedy decode needs H %% 8 == 0 (H=%d)", H);
    if (E < 4 || O < 4 || E > 1024 || O > 1024 || E % 4 || O % 4)
        return fail(RNNT_ERR_UNSUPPORTED, "greedy decode needs 4 <= E, O <= 1024, multiples of 4 (E=%d, O=%d)", E, O);
    *out = align_up(dec_loop_workspace_floats(H, V, E, O, scan_frames) * 4);
    return RNNT_OK;
}

// argument checks shared by the two decode entry points; fills `a` (workspace / iteration fields left to the caller)
static int dec_check_args(const void *frames, int64_t frame_stride, int T, const rnnt_conv_predictor_params *p, int S, int E, int O,
                          float ln_in_eps, float ln_eps, const void *text_W, const void *text_b, const void *W, const void *bias, int H, int V, int blank,
                          int max_length, int max_per_frame, int32_t *host_flag, int32_t *state, int32_t *tokens, void *workspace,
                          DecLoopArgs &a)
{
    int32_t *flag_dev = nullptr;
    if (host_flag) {  // the device's address of the caller's pinned word (an ordinary host pointer is refused, never written through)
        void *dp = nullptr;
        if (hipHostGetDevicePointer(&dp, host_flag, 0) != hipSuccess || !dp) {
            (void)hipGetLastError();
            return fail(RNNT_ERR_INVALID_ARG, "host_flag is not mapped pinned host memory (hipHostMalloc / torch pin_memory)");
        }
        flag_dev = (int32_t *)dp;
    }
    if (!frames || !p || !W || !bias || !state || !tokens || !workspace) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    const void *ptrs[] = {p->embedding, p->ln_in_w, p->ln_in_b, p->conv1_w, p->conv1_b, p->conv2_w, p->conv2_b,
                          p->linear_w, p->linear_b, p->ln_out_w, p->ln_out_b, W, bias, frames};
    for (const void *q : ptrs)
        if (!q || !aligned16(q)) return fail(RNNT_ERR_INVALID_ARG, "null or not 16-byte aligned parameter pointer");
    if ((text_W == nullptr) != (text_b == nullptr) || (text_W && (!aligned16(text_W) || !aligned16(text_b))))
        return fail(RNNT_ERR_INVALID_ARG, "text_W / text_b: both or neither, 16-byte aligned");
    if (!text_W && O != H) return fail(RNNT_ERR_INVALID_ARG, "without text_ln the predictor's output dim (%d) must equal H (%d)", O, H);
    if (T < 1 || S < 1 || max_length < 2 || max_per_frame < 1 || frame_stride < H || frame_stride % 4)
        return fail(RNNT_ERR_INVALID_ARG, "T=%d S=%d max_length=%d max_per_frame=%d frame_stride=%lld", T, S, max_length,
                    max_per_frame, (long long)frame_stride);
    if (blank < 0 || blank >= V) return fail(RNNT_ERR_INVALID_ARG, "blank=%d outside [0,%d)", blank, V);
    if ((uintptr_t)workspace & 255) return fail(RNNT_ERR_INVALID_ARG, "workspace must be 256-byte aligned");
    a.frames = (const float *)frames; a.frame_stride = (long)frame_stride; a.T = T;
    a.p = *p; a.S = S; a.E = E; a.O = O; a.ln_in_eps = ln_in_eps; a.ln_eps = ln_eps;
    a.text_W = (const float *)text_W; a.text_b = (const float *)text_b;
    a.W = (const float *)W; a.bias = (const float *)bias; a.H = H; a.V = V; a.blank = blank;
    a.max_length = max_length; a.max_per_frame = max_per_frame; a.scan_frames = 0; a.iterations = 0; a.init = 1;
    a.host_flag = flag_dev; a.state = state; a.tokens = tokens; a.workspace = workspace;
    return RNNT_OK;
}

int rnnt_engine_greedy_decode(const void *frames, int64_t frame_stride, int T, const rnnt_conv_predictor_params *p,
                              int S, int E, int O, float ln_in_eps, float ln_eps, const void *text_W, const void *text_b,
                              const void *W, const void *bias, int H, int V, int blank, int max_length,
                              int max_per_frame, int scan_frames, int iterations, int init, int32_t *host_flag,
                              int32_t *state, int32_t *tokens, void *workspace, size_t ws_bytes, void *stream)
{
    size_t need;
    if (int rc = rnnt_engine_greedy_decode_workspace_bytes(H, V, E, O, scan_frames, &need)) return rc;
    if (iterations < 0) return fail(RNNT_ERR_INVALID_ARG, "iterations=%d", iterations);
    DecLoopArgs a;
    if (int rc = dec_check_args(frames, frame_stride, T, p, S, E, O, ln_in_eps, ln_eps, text_W, text_b, W, bias, H, V, blank, max_length, max_per_frame,
                                host_flag, state, tokens, workspace, a))
        return rc;
    if (ws_bytes < need) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
    a.scan_frames = scan_frames;
    a.iterations = iterations ? iterations : max_length + (T + scan_frames - 1) / scan_frames + 1;
    a.init = init;
    launch_dec_loop(a, (hipStream_t)stream);
    return launch_status("rnnt_engine_greedy_decode");
}

static int beam_ws_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, bool ctx, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (beam < 1) return fail(RNNT_ERR_INVALID_ARG, "beam=%d must be >= 1", beam);
    if (beam > 16) return fail(RNNT_ERR_UNSUPPORTED, "beam decode takes beam <= 16 (beam=%d)", beam);
    if (S < 1 || max_length < 2) return fail(RNNT_ERR_INVALID_ARG, "S=%d max_length=%d (S >= 1, max_length >= 2)", S, max_length);
    if (max_length > 65536) return fail(RNNT_ERR_UNSUPPORTED, "beam decode takes max_length <= 65536 (max_length=%d)", max_length);
    if (int rc = check_dims(1, 1, 1, H, V, RNNT_DTYPE_F32, true)) return rc;
    if (H % 8 != 0) return fail(RNNT_ERR_UNSUPPORTED, "beam decode needs H %% 8 == 0 (H=%d)", H);
    if (E < 4 || O < 4 || E > 1024 || O > 1024 || E % 4 || O % 4)
        return fail(RNNT_ERR_UNSUPPORTED, "beam decode needs 4 <= E, O <= 1024, multiples of 4 (E=%d, O=%d)", E, O);
    if (!has_text && O != H) return fail(RNNT_ERR_INVALID_ARG, "without text_ln the predictor's output dim (%d) must equal H (%d)", O, H);
    *out = align_up(beam_workspace_bytes(S, E, O, H, V, has_text ? 1 : 0, max_length, ctx));
    return RNNT_OK;
}
int rnnt_engine_beam_decode_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, size_t *out)
{
    return beam_ws_bytes(S, E, O, H, V, has_text, max_length, beam, false, out);
}
int rnnt_engine_beam_decode_ctx_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, size_t *out)
{
    return beam_ws_bytes(S, E, O, H, V, has_text, max_length, beam, true, out);
}

// the context graph of the _ctx entry points: everything the host can see of it (its arrays' contents are the kernels' to distrust)
static int beam_check_ctx(const rnnt_beam_context *g)
{
    if (!g) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument (ctx)");
    if (!g->child_off || !g->child_tok || !g->child_node || !g->fail_link || !g->depth || !g->terminal)
        return fail(RNNT_ERR_INVALID_ARG, "null pointer argument (an array of the context graph)");
    if (g->n_nodes < 1 || g->n_children < 0 || g->n_children >= g->n_nodes)  // (a trie: every node but the root is one child)
        return fail(RNNT_ERR_INVALID_ARG, "context graph: n_nodes=%d n_children=%d (n_nodes >= 1, 0 <= n_children < n_nodes)", g->n_nodes,
                    g->n_children);
    if (g->n_nodes > RNNT_BEAM_CONTEXT_MAX_NODES)
        return fail(RNNT_ERR_UNSUPPORTED, "context graph: n_nodes=%d above %d", g->n_nodes, RNNT_BEAM_CONTEXT_MAX_NODES);
    if (!(g->score >= 0.0) || g->score > 1.7976931348623157e308)
        return fail(RNNT_ERR_INVALID_ARG, "context graph: score=%g must be finite and >= 0", g->score);
    for (const int32_t *a : {g->child_off, g->child_tok, g->child_node, g->fail_link, g->depth, g->terminal})
        if ((uintptr_t)a & 3) return fail(RNNT_ERR_INVALID_ARG, "context graph: arrays must be 4-byte aligned");
    return RNNT_OK;
}

static int beam_decode_any(const void *frames, int64_t frame_stride, int T, const rnnt_conv_predictor_params *p,
                           int S, int E, int O, float ln_in_eps, float ln_out_eps, const void *text_W, const void *text_b,
                           const void *W, const void *bias, int H, int V, int blank, int max_length, int max_per_frame,
                           int beam, const void *tables, int iterations, int init, int32_t *host_flag, int32_t *state,
                           int32_t *tokens, double *scores, void *workspace, size_t ws_bytes, const rnnt_beam_context *ctx, bool with_ctx,
                           void *stream, const char *name)
{
    size_t need;
    if (int rc = beam_ws_bytes(S, E, O, H, V, text_W ? 1 : 0, max_length, beam, with_ctx, &need)) return rc;
    if (with_ctx)
        if (int rc = beam_check_ctx(ctx)) return rc;
    if (iterations < 0) return fail(RNNT_ERR_INVALID_ARG, "iterations=%d", iterations);
    if (!scores) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument (scores)");
    if (tables && !aligned16(tables)) return fail(RNNT_ERR_INVALID_ARG, "tables must be 16-byte aligned");
    if (max_per_frame > 0 && T > 0 && (long)T * max_per_frame + 1 > 0x7fffffffL)
        return fail(RNNT_ERR_UNSUPPORTED, "T * max_per_frame must stay below 2^31 (T=%d, max_per_frame=%d)", T, max_per_frame);
    BeamArgs a;
    if (int rc = dec_check_args(frames, frame_stride, T, p, S, E, O, ln_in_eps, ln_out_eps, text_W, text_b, W, bias, H, V, blank, max_length,
                                max_per_frame, host_flag, state, tokens, workspace, a.d))
        return rc;
    if (ws_bytes < need) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
    a.d.iterations = iterations ? iterations : T * max_per_frame + 1;
    a.d.init = init;
    a.d.tables = tables;
    a.beam = beam;
    a.scores = scores;
    a.ctx = with_ctx ? ctx : nullptr;
    launch_beam_decode(a, (hipStream_t)stream);
    return launch_status(name);
}
int rnnt_engine_beam_decode(const void *frames, int64_t frame_stride, int T, const rnnt_conv_predictor_params *p,
                            int S, int E, int O, float ln_in_eps, float ln_out_eps, const void *text_W, const void *text_b,
                            const void *W, const void *bias, int H, int V, int blank, int max_length, int max_per_frame,
                            int beam, const void *tables, int iterations, int init, int32_t *host_flag, int32_t *state,
                            int32_t *tokens, double *scores, void *workspace, size_t ws_bytes, void *stream)
{
    return beam_decode_any(frames, frame_stride, T, p, S, E, O, ln_in_eps, ln_out_eps, text_W, text_b, W, bias, H, V, blank, max_length,
                           max_per_frame, beam, tables, iterations, init, host_flag, state, tokens, scores, workspace, ws_bytes, nullptr, false,
                           stream, "rnnt_engine_beam_decode");
}
int rnnt_engine_beam_decode_ctx(const void *frames, int64_t frame_stride, int T, const rnnt_conv_predictor_params *p,
                                int S, int E, int O, float ln_in_eps, float ln_out_eps, const void *text_W, const void *text_b,
                                const void *W, const void *bias, int H, int V, int blank, int max_length, int max_per_frame,
                                int beam, const void *tables, int iterations, int init, int32_t *host_flag, int32_t *state,
                                int32_t *tokens, double *scores, void *workspace, size_t ws_bytes, const rnnt_beam_context *ctx,
                                void *stream)
{
    return beam_decode_any(frames, frame_stride, T, p, S, E, O, ln_in_eps, ln_out_eps, text_W, text_b, W, bias, H, V, blank, max_length,
                           max_per_frame, beam, tables, iterations, init, host_flag, state, tokens, scores, workspace, ws_bytes, ctx, true,
                           stream, "rnnt_engine_beam_decode_ctx");
}

static int beam_batch_ws_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, int n_utt, bool ctx, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (n_utt < 1 || n_utt > 64) return fail(RNNT_ERR_UNSUPPORTED, "batched beam decode takes 1 <= n_utt <= 64 (n_utt=%d)", n_utt);
    if (int rc = beam_ws_bytes(S, E, O, H, V, has_text, max_length, beam, ctx, out)) return rc;
    *out = align_up(beam_batch_workspace_bytes(S, E, O, H, V, has_text ? 1 : 0, max_length, n_utt, ctx));
    return RNNT_OK;
}
int rnnt_engine_beam_decode_batch_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, int n_utt,
                                                  size_t *out)
{
    return beam_batch_ws_bytes(S, E, O, H, V, has_text, max_length, beam, n_utt, false, out);
}
int rnnt_engine_beam_decode_batch_ctx_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam,
                                                      int n_utt, size_t *out)
{
    return beam_batch_ws_bytes(S, E, O, H, V, has_text, max_length, beam, n_utt, true, out);
}

static int beam_decode_batch_any(const void *frames, int64_t frame_stride, int rows, const int32_t *utt, int n_utt, int max_frames,
                                 const rnnt_conv_predictor_params *p, int S, int E, int O, float ln_in_eps, float ln_out_eps,
                                 const void *text_W, const void *text_b, const void *W, const void *bias, int H, int V, int blank,
                                 int max_length, int max_per_frame, int beam, const void *tables, int iterations, int init,
                                 int32_t *host_flag, int32_t *state, int32_t *tokens, double *scores, void *workspace, size_t ws_bytes,
                                 const rnnt_beam_context *ctx, bool with_ctx, void *stream, const char *name)
{
    size_t need;
    if (int rc = beam_batch_ws_bytes(S, E, O, H, V, text_W ? 1 : 0, max_length, beam, n_utt, with_ctx, &need)) return rc;
    if (with_ctx)
        if (int rc = beam_check_ctx(ctx)) return rc;
    if (iterations < 0) return fail(RNNT_ERR_INVALID_ARG, "iterations=%d", iterations);
    if (!scores || !utt) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument (scores / utt)");
    if ((uintptr_t)utt & 7) return fail(RNNT_ERR_INVALID_ARG, "utt must be 8-byte aligned");
    if (tables && !aligned16(tables)) return fail(RNNT_ERR_INVALID_ARG, "tables must be 16-byte aligned");
    if (max_frames < 1 || rows < max_frames)
        return fail(RNNT_ERR_INVALID_ARG, "rows=%d max_frames=%d (1 <= max_frames <= rows)", rows, max_frames);
    if (max_per_frame > 0 && (long)max_frames * max_per_frame + 1 > 0x7fffffffL)
        return fail(RNNT_ERR_UNSUPPORTED, "max_frames * max_per_frame must stay below 2^31 (max_frames=%d, max_per_frame=%d)", max_frames,
                    max_per_frame);
    BeamArgs a;
    if (int rc = dec_check_args(frames, frame_stride, max_frames, p, S, E, O, ln_in_eps, ln_out_eps, text_W, text_b, W, bias, H, V, blank,
                                max_length, max_per_frame, host_flag, state, tokens, workspace, a.d))
        return rc;
    if (ws_bytes < need) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
    a.d.iterations = iterations ? iterations : max_frames * max_per_frame + 1;
    a.d.init = init;
    a.d.tables = tables;
    a.beam = beam;
    a.scores = scores;
    a.utt = utt; a.n_utt = n_utt; a.rows = rows;
    a.ctx = with_ctx ? ctx : nullptr;
    launch_beam_decode(a, (hipStream_t)stream);
    return launch_status(name);
}
int rnnt_engine_beam_decode_batch(const void *frames, int64_t frame_stride, int rows, const int32_t *utt, int n_utt, int max_frames,
                                  const rnnt_conv_predictor_params *p, int S, int E, int O, float ln_in_eps, float ln_out_eps,
                                  const void *text_W, const void *text_b, const void *W, const void *bias, int H, int V, int blank,
                                  int max_length, int max_per_frame, int beam, const void *tables, int iterations, int init,
                                  int32_t *host_flag, int32_t *state, int32_t *tokens, double *scores, void *workspace, size_t ws_bytes,
                                  void *stream)
{
    return beam_decode_batch_any(frames, frame_stride, rows, utt, n_utt, max_frames, p, S, E, O, ln_in_eps, ln_out_eps, text_W, text_b, W, bias,
                                 H, V, blank, max_length, max_per_frame, beam, tables, iterations, init, host_flag, state, tokens, scores,
                                 workspace, ws_bytes, nullptr, false, stream, "rnnt_engine_beam_decode_batch");
}
int rnnt_engine_beam_decode_batch_ctx(const void *frames, int64_t frame_stride, int rows, const int32_t *utt, int n_utt, int max_frames,
                                      const rnnt_conv_predictor_params *p, int S, int E, int O, float ln_in_eps, float ln_out_eps,
                                      const void *text_W, const void *text_b, const void *W, const void *bias, int H, int V, int blank,
                                      int max_length, int max_per_frame, int beam, const void *tables, int iterations, int init,
                                      int32_t *host_flag, int32_t *state, int32_t *tokens, double *scores, void *workspace,
                                      size_t ws_bytes, const rnnt_beam_context *ctx, void *stream)
{
    return beam_decode_batch_any(frames, frame_stride, rows, utt, n_utt, max_frames, p, S, E, O, ln_in_eps, ln_out_eps, text_W, text_b, W, bias,
                                 H, V, blank, max_length, max_per_frame, beam, tables, iterations, init, host_flag, state, tokens, scores,
                                 workspace, ws_bytes, ctx, true, stream, "rnnt_engine_beam_decode_batch_ctx");
}

int rnnt_engine_beam_stream_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, int n_streams, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (n_streams < 1 || n_streams > 64) return fail(RNNT_ERR_UNSUPPORTED, "beam streams: 1 <= n_streams <= 64 (n_streams=%d)", n_streams);
    if (int rc = rnnt_engine_beam_decode_workspace_bytes(S, E, O, H, V, has_text, max_length, beam, out)) return rc;
    *out = align_up(beam_stream_block_bytes(S, E, O, H, V, has_text ? 1 : 0, max_length, n_streams));
    return RNNT_OK;
}

int rnnt_engine_beam_stream_init(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, int blank, int n_streams,
                                 int index, int32_t *state, double *scores, void *block, size_t bytes, void *stream)
{
    size_t need;
    if (int rc = rnnt_engine_beam_stream_bytes(S, E, O, H, V, has_text, max_length, beam, n_streams, &need)) return rc;
    if (!state || !scores || !block) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    if (index < -1 || index >= n_streams) return fail(RNNT_ERR_INVALID_ARG, "index=%d outside [-1,%d)", index, n_streams);
    if (blank < 0 || blank >= V) return fail(RNNT_ERR_INVALID_ARG, "blank=%d outside [0,%d)", blank, V);
    if ((uintptr_t)block & 255) return fail(RNNT_ERR_INVALID_ARG, "block must be 256-byte aligned");
    if (bytes < need) return fail(RNNT_ERR_WORKSPACE, "stream block (workspace) %zu < required %zu bytes", bytes, need);
    launch_beam_stream_init(block, state, scores, S, E, O, H, V, has_text ? 1 : 0, max_length, beam, blank, n_streams, index < 0 ? 0 : index,
                            index < 0 ? n_streams : 1, (hipStream_t)stream);
    return launch_status("rnnt_engine_beam_stream_init");
}

int rnnt_engine_beam_stream_push(const void *frames, int64_t frame_stride, int rows, const int32_t *push_table, int n_streams, int max_count,
                                 const rnnt_conv_predictor_params *p, int S, int E, int O, float ln_in_eps, float ln_out_eps,
                                 const void *text_W, const void *text_b, const void *W, const void *bias, int H, int V, int blank,
                                 int max_length, int max_per_frame, int beam, const void *tables, int iterations, int begin,
                                 int32_t *host_flag, int32_t *state, int32_t *tokens, double *scores, void *block, size_t bytes,
                                 void *stream)
{
    size_t need;
    if (int rc = rnnt_engine_beam_stream_bytes(S, E, O, H, V, text_W ? 1 : 0, max_length, beam, n_streams, &need)) return rc;
    if (iterations < 0) return fail(RNNT_ERR_INVALID_ARG, "iterations=%d", iterations);
    if (!scores || !push_table || !tables) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument (scores / push_table / tables)");
    if ((uintptr_t)push_table & 7) return fail(RNNT_ERR_INVALID_ARG, "push_table must be 8-byte aligned");
    if (!aligned16(tables)) return fail(RNNT_ERR_INVALID_ARG, "tables must be 16-byte aligned");
    if (max_count < 0 || rows < 1 || rows < max_count)
        return fail(RNNT_ERR_INVALID_ARG, "rows=%d max_count=%d (0 <= max_count <= rows, rows >= 1)", rows, max_count);
    if (max_per_frame > 0 && (long)max_count * max_per_frame + 1 > 0x7fffffffL)
        return fail(RNNT_ERR_UNSUPPORTED, "max_count * max_per_frame must stay below 2^31 (max_count=%d, max_per_frame=%d)", max_count,
                    max_per_frame);
    BeamArgs a;
    if (int rc = dec_check_args(frames, frame_stride, max_count > 0 ? max_count : 1, p, S, E, O, ln_in_eps, ln_out_eps, text_W, text_b, W, bias, H, V,
                                blank, max_length, max_per_frame, host_flag, state, tokens, block, a.d))
        return rc;
    if (bytes < need) return fail(RNNT_ERR_WORKSPACE, "stream block (workspace) %zu < required %zu bytes", bytes, need);
    a.d.iterations = iterations ? iterations : max_count * max_per_frame + 1;
    a.d.init = begin;
    a.d.tables = tables;
    a.beam = beam;
    a.scores = scores;
    a.utt = push_table; a.n_utt = n_streams; a.rows = rows;
    a.streaming = true;
    launch_beam_decode(a, (hipStream_t)stream);
    return launch_status("rnnt_engine_beam_stream_push");
}

static int dec_persist_check(int T, int S, int E, int O, int H, int V, int has_text, int max_length)
{
    if (int rc = check_dims(1, 16, 1, H, V, RNNT_DTYPE_F32, true)) return rc;
    if (const char *why = dec_persist_refusal(T, S, E, O, H, V, has_text))
        return fail(RNNT_ERR_UNSUPPORTED, "persistent greedy decode: %s (T=%d S=%d E=%d O=%d H=%d V=%d)", why, T, S, E, O, H, V);
    if ((long)T + max_length + 2 >= (1L << 20)) return fail(RNNT_ERR_UNSUPPORTED, "persistent greedy decode: T + max_length must stay below 2^20");
    // the kernel keeps 100-138 KB in LDS: a device with less (not a gfx950) is "unsupported", so that callers take the kernel-per-layer loop
    // instead of a failed launch.  Without a device (size queries on a CPU-only host) there is nothing to check against.
    int dev = 0, lds_max = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess) {
        if (dec_persist_lds_bytes(E) > (size_t)lds_max)
            return fail(RNNT_ERR_UNSUPPORTED, "persistent greedy decode needs %zu bytes of LDS per workgroup, the device allows %d",
                        dec_persist_lds_bytes(E), lds_max);
    } else {
        (void)hipGetLastError();
    }
    return RNNT_OK;
}

int rnnt_engine_greedy_decode_persistent_workspace_bytes(int T, int S, int E, int O, int H, int V, int has_text, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (T < 1 || S < 1) return fail(RNNT_ERR_INVALID_ARG, "T=%d S=%d", T, S);
    if (int rc = dec_persist_check(T, S, E, O, H, V, has_text, 2)) return rc;
    *out = align_up(dec_persist_workspace_floats(T, S, E, O, H, V, has_text) * 4);
    return RNNT_OK;
}

int rnnt_engine_greedy_decode_tables_bytes(int S, int E, int O, int H, int has_text, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (S < 1) return fail(RNNT_ERR_INVALID_ARG, "S=%d", S);
    // (the tables do not depend on V or T.)  S: the persistent loop's limit of 4096 symbols is that loop's own — its size query states it —
    // and not the tables': the batched and the streaming beam search bring them too and take any S, as the single search does, which
    // builds them in its workspace
    if (int rc = dec_persist_check(8, S > 4096 ? 4096 : S, E, O, H, 1024, has_text, 2)) return rc;
    *out = align_up(dec_tables_floats(S, E, O, H, has_text) * 4);
    return RNNT_OK;
}

int rnnt_engine_greedy_decode_build_tables(const rnnt_conv_predictor_params *p, int S, int E, int O, float ln_in_eps, const void *text_W,
                                           const void *text_b, int H, void *tables, size_t tables_bytes, void *stream)
{
    size_t need;
    if (int rc = rnnt_engine_greedy_decode_tables_bytes(S, E, O, H, text_W ? 1 : 0, &need)) return rc;
    if (!p || !tables) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    const void *ptrs[] = {p->embedding, p->ln_in_w, p->ln_in_b, p->conv1_w, p->conv1_b, p->conv2_w, p->conv2_b,
                          p->linear_w, p->linear_b, p->ln_out_w, p->ln_out_b};
    for (const void *q : ptrs)
        if (!q || !aligned16(q)) return fail(RNNT_ERR_INVALID_ARG, "null or not 16-byte aligned parameter pointer");
    if ((text_W == nullptr) != (text_b == nullptr) || (text_W && (!aligned16(text_W) || !aligned16(text_b))))
        return fail(RNNT_ERR_INVALID_ARG, "text_W / text_b: both or neither, 16-byte aligned");
    if (!text_W && O != H) return fail(RNNT_ERR_INVALID_ARG, "without text_ln the predictor's output dim (%d) must equal H (%d)", O, H);
    if ((uintptr_t)tables & 255) return fail(RNNT_ERR_INVALID_ARG, "tables must be 256-byte aligned");
    if (tables_bytes < need) return fail(RNNT_ERR_WORKSPACE, "tables %zu < required %zu bytes", tables_bytes, need);
    launch_dec_build_tables(*p, S, E, O, ln_in_eps, (const float *)text_W, (const float *)text_b, H, (float *)tables, (hipStream_t)stream);
    return launch_status("rnnt_engine_greedy_decode_build_tables");
}

int rnnt_engine_greedy_decode_persistent(const void *frames, int64_t frame_stride, int T, const rnnt_conv_predictor_params *p,
                                         int S, int E, int O, float ln_in_eps, float ln_eps, const void *text_W, const void *text_b,
                                         const void *W, const void *bias, int H, int V, int blank, int max_length,
                                         int max_per_frame, const void *tables, int32_t *host_flag, int32_t *state, int32_t *tokens,
                                         void *workspace, size_t ws_bytes, void *stream)
{
    if (T < 1 || S < 1 || max_length < 2) return fail(RNNT_ERR_INVALID_ARG, "T=%d S=%d max_length=%d", T, S, max_length);
    if (int rc = dec_persist_check(T, S, E, O, H, V, text_W ? 1 : 0, max_length)) return rc;
    DecLoopArgs a;
    if (int rc = dec_check_args(frames, frame_stride, T, p, S, E, O, ln_in_eps, ln_eps, text_W, text_b, W, bias, H, V, blank, max_length, max_per_frame,
                                host_flag, state, tokens, workspace, a))
        return rc;
    const size_t need = align_up(dec_persist_workspace_floats(T, S, E, O, H, V, text_W ? 1 : 0) * 4);
    if (ws_bytes < need) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return fail(RNNT_ERR_LAUNCH, "cannot query the device's compute-unit count");
    if (dec_persist_groups(V) > cus)  // the loop's workgroups wait for each other: all of them must be resident
        return fail(RNNT_ERR_UNSUPPORTED, "persistent greedy decode needs %d compute units, the device has %d", dec_persist_groups(V), cus);
    if (tables && ((uintptr_t)tables & 255)) return fail(RNNT_ERR_INVALID_ARG, "tables must be 256-byte aligned");
    a.tables = tables;
    if (const int e = launch_dec_persist(a, (hipStream_t)stream))
        return fail(RNNT_ERR_LAUNCH, "persistent greedy decode: cannot raise the kernel's dynamic LDS limit to %zu bytes: %s",
                    dec_persist_lds_bytes(E), hipGetErrorString((hipError_t)e));
    return launch_status("rnnt_engine_greedy_decode_persistent");
}

int rnnt_engine_greedy_stream_init(int32_t *state, int blank, void *stream)
{
    if (!state) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument (state)");
    if (((uintptr_t)state & 3) || blank < 0) return fail(RNNT_ERR_INVALID_ARG, "state must be 4-byte aligned, blank >= 0 (blank=%d)", blank);
    launch_stream_init(state, blank, (hipStream_t)stream);
    return launch_status("rnnt_engine_greedy_stream_init");
}

// the labels a push may emit: n * max_per_frame, fewer when max_length leaves fewer
static long stream_cap(int n, int max_length, int max_per_frame)
{
    const long cap = (long)n * max_per_frame;
    return max_length > 0 ? std::min(cap, (long)max_length - 1) : cap;
}

int rnnt_engine_greedy_stream_decode_workspace_bytes(int n, int S, int E, int O, int H, int V, int has_text, int max_length,
                                                     int max_per_frame, int persistent, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null size pointer");
    if (n < 0 || S < 1 || max_per_frame < 1 || max_length < 0 || max_length == 1 || (persistent != 0 && persistent != 1))
        return fail(RNNT_ERR_INVALID_ARG, "stream decode: n=%d S=%d max_length=%d max_per_frame=%d persistent=%d (n >= 0, S >= 1, "
                    "max_length 0 or >= 2, max_per_frame >= 1, persistent 0 or 1)", n, S, max_length, max_per_frame, persistent);
    if ((long)n * max_per_frame >= (1L << 30))
        return fail(RNNT_ERR_UNSUPPORTED, "stream decode: n * max_per_frame must stay below 2^30 (n=%d, max_per_frame=%d)", n, max_per_frame);
    if (!has_text && O != H) return fail(RNNT_ERR_INVALID_ARG, "without text_ln the predictor's output dim (%d) must equal H (%d)", O, H);
    size_t loop_bytes;  // the kernel-per-layer loop's own checks (sizes)
    if (int rc = rnnt_engine_greedy_decode_workspace_bytes(H, V, E, O, 32, &loop_bytes)) return rc;
    const long cap = stream_cap(n, max_length, max_per_frame);
    if (persistent) {
        if (int rc = dec_persist_check(n < 1 ? 1 : n, S, E, O, H, V, has_text, 2)) return rc;
        if ((long)n + cap + 2 >= (1L << 20)) return fail(RNNT_ERR_UNSUPPORTED, "persistent stream decode: n + labels per push must stay below 2^20");
    }
    *out = align_up(dec_stream_workspace_bytes(n, S, E, O, H, V, has_text ? 1 : 0, (int)cap, persistent));
    return RNNT_OK;
}

int rnnt_engine_greedy_stream_decode(const void *frames, int64_t frame_stride, int n, const rnnt_conv_predictor_params *p,
                                     int S, int E, int O, float ln_in_eps, float ln_out_eps, const void *text_W, const void *text_b,
                                     const void *W, const void *bias, int H, int V, int blank, int max_length, int max_per_frame,
                                     const void *tables, int persistent, int32_t *state, int32_t *out_tokens, void *workspace,
                                     size_t ws_bytes, void *stream)
{
    size_t need;
    if (int rc = rnnt_engine_greedy_stream_decode_workspace_bytes(n, S, E, O, H, V, text_W ? 1 : 0, max_length, max_per_frame, persistent, &need))
        return rc;
    if (!state || !out_tokens || (n > 0 && !frames)) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument (frames, state or out_tokens)");
    if (((uintptr_t)state & 3) || ((uintptr_t)out_tokens & 3)) return fail(RNNT_ERR_INVALID_ARG, "state and out_tokens must be 4-byte aligned");
    if (tables && ((uintptr_t)tables & 255)) return fail(RNNT_ERR_INVALID_ARG, "tables must be 256-byte aligned");
    DecLoopArgs a;  // (an empty push has no frames: the checks look at W in their place)
    if (int rc = dec_check_args(n > 0 ? frames : W, frame_stride, n > 0 ? n : 1, p, S, E, O, ln_in_eps, ln_out_eps, text_W, text_b, W, bias, H, V,
                                blank, max_length > 0 ? max_length : 2, max_per_frame, nullptr, state, out_tokens, workspace, a))
        return rc;
    if (ws_bytes < need) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
    if (persistent && n > 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            return fail(RNNT_ERR_LAUNCH, "cannot query the device's compute-unit count");
        if (dec_persist_groups(V) > cus)
            return fail(RNNT_ERR_UNSUPPORTED, "persistent stream decode needs %d compute units, the device has %d", dec_persist_groups(V), cus);
    }
    a.frames = n > 0 ? (const float *)frames : nullptr;
    a.T = n;
    a.max_length = max_length;
    a.stream_cap = (int)stream_cap(n, max_length, max_per_frame);
    a.sstate = state;
    a.tables = tables;
    if (const int e = launch_dec_stream(a, persistent, (hipStream_t)stream))
        return fail(RNNT_ERR_LAUNCH, "persistent stream decode: cannot raise the kernel's dynamic LDS limit to %zu bytes: %s",
                    dec_persist_lds_bytes(E), hipGetErrorString((hipError_t)e));
    return launch_status("rnnt_engine_greedy_stream_decode");
}

static int loss_fwd_bwd(const void *logits, const int32_t *targets, const int32_t *logit_lens,
                        const int32_t *target_lens, int B, int T, int U1, int V, int blank, float clamp,
                        float fastemit, float delay, int dtype, float *costs, void *grad_logits,
                        void *workspace, size_t ws_bytes, void *stream, const int32_t *restrict_frames = nullptr,
                        int restrict_left = 0, int restrict_right = 0)
{
    if (int rc = check_dims(B, T, U1, 4, V, dtype, false)) return rc;
    if (!logits || !targets || !logit_lens || !target_lens || !costs || !workspace)
        return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    if (blank < 0 || blank >= V) return fail(RNNT_ERR_INVALID_ARG, "blank=%d outside [0,%d)", blank, V);
    if (!aligned16(logits) || (grad_logits && !aligned16(grad_logits)) || ((uintptr_t)workspace & 255))
        return fail(RNNT_ERR_INVALID_ARG, "pointers must be 16-byte aligned (workspace 256)");
    size_t need;
    rnnt_engine_loss_workspace_bytes(B, T, U1, V, dtype, &need);
    if (ws_bytes < need) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
    LossCall c{};
    loss_call(c, workspace, targets, logit_lens, target_lens, costs, B, T, U1, grad_logits ? ST_LATTICE | ST_COEF : ST_LATTICE, 1.0f,
              fastemit, delay, (hipStream_t)stream, restrict_frames, restrict_left, restrict_right);
    c.logits = (const float *)logits; c.grad_logits = (float *)grad_logits; c.V = V; c.blank = blank; c.clamp = clamp;
    launch_logsoftmax_gather(c, c.st);
    loss_stages(c);
    if (grad_logits) launch_grad_logits(c, c.st);
    return launch_status("rnnt_engine_loss_fwd_bwd");
}

int rnnt_engine_loss_fwd_bwd(const void *logits, const int32_t *targets, const int32_t *logit_lens,
                             const int32_t *target_lens, int B, int T, int U1, int V, int blank,
                             float clamp, int dtype, float *costs, void *grad_logits,
                             void *workspace, size_t ws_bytes, void *stream)
{
    return loss_fwd_bwd(logits, targets, logit_lens, target_lens, B, T, U1, V, blank, clamp, 0.f, 0.f, dtype,
                        costs, grad_logits, workspace, ws_bytes, stream);
}

// ---- FastEmit and the delay penalty: the entries above with the two options added
int rnnt_engine_loss_fwd_bwd_reg(const void *logits, const int32_t *targets, const int32_t *logit_lens,
                                 const int32_t *target_lens, int B, int T, int U1, int V, int blank,
                                 float clamp, float fastemit_lambda, float delay_penalty, int dtype,
                                 float *costs, void *grad_logits, void *workspace, size_t ws_bytes,
                                 void *stream)
{
    if (int rc = check_reg(fastemit_lambda, delay_penalty)) return rc;
    return loss_fwd_bwd(logits, targets, logit_lens, target_lens, B, T, U1, V, blank, clamp, fastemit_lambda,
                        delay_penalty, dtype, costs, grad_logits, workspace, ws_bytes, stream);
}

int rnnt_engine_joint_loss_fwd_bwd_reg(const void *enc, const int64_t enc_strides[3], const void *pred,
                                       const void *W, const void *bias, const int32_t *targets,
                                       const int32_t *logit_lens, const int32_t *target_lens, int B,
                                       int T, int U1, int H, int V, int blank, float clamp,
                                       float grad_scale, float fastemit_lambda, float delay_penalty,
                                       int dtype, float *costs, void *grad_enc, void *grad_pred,
                                       void *grad_W, void *grad_bias, void *workspace, size_t ws_bytes,
                                       void *stream)
{
    if (int rc = check_reg(fastemit_lambda, delay_penalty)) return rc;
    // (the f16x2 route's flush rule is not extended to the regularised coefficients: nothing is flushed here, whatever the options)
    return run_fused(ST_ALL, RNNT_VARIANT_X2_NO_FLUSH_SKIP, enc, enc_strides, pred, W, bias, targets, logit_lens, target_lens, B, T,
                     U1, H, V, blank, clamp, grad_scale, fastemit_lambda, delay_penalty, dtype, costs,
                     grad_enc, grad_pred, grad_W, grad_bias, workspace, ws_bytes, stream);
}

int rnnt_engine_joint_loss_fwd_reg(const void *enc, const int64_t enc_strides[3], const void *pred,
                                   const void *W, const void *bias, const int32_t *targets,
                                   const int32_t *logit_lens, const int32_t *target_lens, int B, int T,
                                   int U1, int H, int V, int blank, float delay_penalty, int dtype,
                                   float *costs, void *workspace, size_t ws_bytes, void *stream)
{
    if (int rc = check_reg(0.f, delay_penalty)) return rc;
    return run_fused(ST_PROD | ST_FWD | ST_LATTICE, 0, enc, enc_strides, pred, W, bias, targets, logit_lens,
                     target_lens, B, T, U1, H, V, blank, -1.0f, 1.0f, 0.f, delay_penalty, dtype, costs, nullptr,
                     nullptr, nullptr, nullptr, workspace, ws_bytes, stream);
}

// ---- alignment-restricted loss: the *_reg entries with the label arcs confined to a window around restrict_frames.
// f16x2: the flush rule stays on (dead cells are skipped either way) unless an option of §4k is on, as in the *_reg entry.
int rnnt_engine_loss_fwd_bwd_restrict(const void *logits, const int32_t *targets, const int32_t *logit_lens,
                                      const int32_t *target_lens, int B, int T, int U1, int V, int blank,
                                      float clamp, float fastemit_lambda, float delay_penalty,
                                      const int32_t *restrict_frames, int restrict_left, int restrict_right,
                                      int dtype, float *costs, void *grad_logits, void *workspace,
                                      size_t ws_bytes, void *stream)
{
    if (int rc = check_reg(fastemit_lambda, delay_penalty)) return rc;
    if (int rc = check_restrict(restrict_frames, restrict_left, restrict_right)) return rc;
    return loss_fwd_bwd(logits, targets, logit_lens, target_lens, B, T, U1, V, blank, clamp, fastemit_lambda,
                        delay_penalty, dtype, costs, grad_logits, workspace, ws_bytes, stream, restrict_frames,
                        restrict_left, restrict_right);
}

int rnnt_engine_joint_loss_fwd_bwd_restrict(const void *enc, const int64_t enc_strides[3], const void *pred,
                                            const void *W, const void *bias, const int32_t *targets,
                                            const int32_t *logit_lens, const int32_t *target_lens, int B,
                                            int T, int U1, int H, int V, int blank, float clamp,
                                            float grad_scale, float fastemit_lambda, float delay_penalty,
                                            const int32_t *restrict_frames, int restrict_left,
                                            int restrict_right, int dtype, float *costs, void *grad_enc,
                                            void *grad_pred, void *grad_W, void *grad_bias, void *workspace,
                                            size_t ws_bytes, void *stream)
{
    if (int rc = check_reg(fastemit_lambda, delay_penalty)) return rc;
    if (int rc = check_restrict(restrict_frames, restrict_left, restrict_right)) return rc;
    return run_fused(ST_ALL, 0, enc, enc_strides, pred, W, bias, targets, logit_lens, target_lens, B, T, U1, H, V, blank,
                     clamp, grad_scale, fastemit_lambda, delay_penalty, dtype, costs, grad_enc, grad_pred, grad_W,
                     grad_bias, workspace, ws_bytes, stream, restrict_frames, restrict_left, restrict_right);
}

int rnnt_engine_joint_loss_fwd_restrict(const void *enc, const int64_t enc_strides[3], const void *pred,
                                        const void *W, const void *bias, const int32_t *targets,
                                        const int32_t *logit_lens, const int32_t *target_lens, int B, int T,
                                        int U1, int H, int V, int blank, float delay_penalty,
                                        const int32_t *restrict_frames, int restrict_left, int restrict_right,
                                        int dtype, float *costs, void *workspace, size_t ws_bytes,
                                        void *stream)
{
    if (int rc = check_reg(0.f, delay_penalty)) return rc;
    if (int rc = check_restrict(restrict_frames, restrict_left, restrict_right)) return rc;
    return run_fused(ST_PROD | ST_FWD | ST_LATTICE, 0, enc, enc_strides, pred, W, bias, targets, logit_lens,
                     target_lens, B, T, U1, H, V, blank, -1.0f, 1.0f, 0.f, delay_penalty, dtype, costs, nullptr,
                     nullptr, nullptr, nullptr, workspace, ws_bytes, stream, restrict_frames, restrict_left,
                     restrict_right);
}

int rnnt_engine_joint_loss_fwd_bwd(const void *enc, const int64_t enc_strides[3], const void *pred,
                                   const void *W, const void *bias, const int32_t *targets,
                                   const int32_t *logit_lens, const int32_t *target_lens, int B,
                                   int T, int U1, int H, int V, int blank, float clamp,
                                   float grad_scale, int dtype, float *costs, void *grad_enc,
                                   void *grad_pred, void *grad_W, void *grad_bias, void *workspace,
                                   size_t ws_bytes, void *stream)
{
    return run_fused(ST_ALL, 0, enc, enc_strides, pred, W, bias, targets, logit_lens, target_lens, B, T,
                     U1, H, V, blank, clamp, grad_scale, 0.f, 0.f, dtype, costs, grad_enc, grad_pred, grad_W,
                     grad_bias, workspace, ws_bytes, stream);
}

int rnnt_engine_joint_loss_fwd(const void *enc, const int64_t enc_strides[3], const void *pred,
                               const void *W, const void *bias, const int32_t *targets,
                               const int32_t *logit_lens, const int32_t *target_lens, int B, int T,
                               int U1, int H, int V, int blank, int dtype, float *costs,
                               void *workspace, size_t ws_bytes, void *stream)
{
    return run_fused(ST_PROD | ST_FWD | ST_LATTICE, 0, enc, enc_strides, pred, W, bias, targets, logit_lens,
                     target_lens, B, T, U1, H, V, blank, -1.0f, 1.0f, 0.f, 0.f, dtype, costs, nullptr, nullptr,
                     nullptr, nullptr, workspace, ws_bytes, stream);
}

// ---- forced alignment: the loss's producers fill lp_blank / lp_emit, then the Viterbi sweep and the
// backtrace of align.hip.  The backpointer words take the alpha_s region, which the alignment does not use for alpha.
int rnnt_engine_align(const void *logits, const int32_t *targets, const int32_t *logit_lens,
                      const int32_t *target_lens, int B, int T, int U1, int V, int blank,
                      float *scores, int32_t *frames, void *workspace, size_t ws_bytes, void *stream)
{
    if (int rc = check_dims(B, T, U1, 4, V, RNNT_DTYPE_F32, false)) return rc;
    if (!logits || !targets || !logit_lens || !target_lens || !scores || !frames || !workspace)
        return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    if (blank < 0 || blank >= V) return fail(RNNT_ERR_INVALID_ARG, "blank=%d outside [0,%d)", blank, V);
    if (!aligned16(logits) || ((uintptr_t)workspace & 255))
        return fail(RNNT_ERR_INVALID_ARG, "pointers must be 16-byte aligned (workspace 256)");
    size_t need;
    rnnt_engine_loss_workspace_bytes(B, T, U1, V, RNNT_DTYPE_F32, &need);
    if (ws_bytes < need) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
    LossCall c{};  // the loss entry's layout; the backpointer words take the alpha_s region
    loss_call(c, workspace, targets, logit_lens, target_lens, scores, B, T, U1, 0, 1.0f, 0.f, 0.f, (hipStream_t)stream, nullptr, 0, 0);
    c.logits = (const float *)logits; c.V = V; c.blank = blank;
    launch_logsoftmax_gather(c, c.st);
    launch_align(c, c.alpha_s, scores, frames, c.st);
    return launch_status("rnnt_engine_align");
}

int rnnt_engine_joint_align(const void *enc, const int64_t enc_strides[3], const void *pred,
                            const void *W, const void *bias, const int32_t *targets,
                            const int32_t *logit_lens, const int32_t *target_lens, int B, int T,
                            int U1, int H, int V, int blank, int dtype, float *scores,
                            int32_t *frames, void *workspace, size_t ws_bytes, void *stream)
{
    if (!scores || !frames) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    // operand producers + the joint-forward GEMM (log-softmax in its epilogue) of the loss; every
    // argument is checked there before anything is enqueued
    if (int rc = run_fused(ST_PROD | ST_FWD, 0, enc, enc_strides, pred, W, bias, targets, logit_lens,
                           target_lens, B, T, U1, H, V, blank, -1.0f, 1.0f, 0.f, 0.f, dtype, scores, nullptr,
                           nullptr, nullptr, nullptr, workspace, ws_bytes, stream))
        return rc;
    rnnt_engine_ws_layout L;
    layout(B, T, U1, H, V, dtype, &L);
    LossCall c{};
    loss_call(c, (char *)workspace + L.denom_s, targets, logit_lens, target_lens, scores, B, T, U1, 0, 1.0f, 0.f, 0.f, (hipStream_t)stream,
              nullptr, 0, 0);
    launch_align(c, c.alpha_s, scores, frames, c.st);
    return launch_status("rnnt_engine_joint_align");
}

// ---- CTC auxiliary head (ctc.hip).  The workspace: denom | lp_blank | lp_label | alpha | beta | links | log P | err
static int ctc_check_dims(int N, int T, int U, int V)
{
    if (N <= 0 || T <= 0 || V <= 0 || U < 0) return fail(RNNT_ERR_INVALID_ARG, "non-positive dimension N=%d T=%d U=%d V=%d", N, T, U, V);
    if (V % 4 != 0) return fail(RNNT_ERR_UNSUPPORTED, "V=%d must be a multiple of 4 (pad on the host side)", V);
    if (U > 1023) return fail(RNNT_ERR_UNSUPPORTED, "U=%d exceeds 1023 labels (two CTC states per lane of a 1024-thread workgroup)", U);
    return RNNT_OK;
}

static size_t ctc_carve(void *ws, int N, int T, int U, CtcArgs *a)
{
    const size_t rows = (size_t)N * T, Us = U > 0 ? U : 1, S2 = 2 * ((size_t)U + 1);
    const size_t r4 = align_up(rows * 4), l4 = align_up(rows * Us * 4), s8 = align_up(rows * S2 * 8);
    const size_t lk = align_up((size_t)N * Us * 4), lp = align_up((size_t)N * 8);
    if (a) {
        const uintptr_t p = (uintptr_t)ws;
        a->denom = (float *)p; a->lpb = (float *)(p + r4); a->lpl = (float *)(p + 2 * r4);
        a->alpha = (double *)(p + 2 * r4 + l4); a->beta = (double *)(p + 2 * r4 + l4 + s8);
        a->link = (int32_t *)(p + 2 * r4 + l4 + 2 * s8); a->logp = (double *)(p + 2 * r4 + l4 + 2 * s8 + lk);
        a->err = (unsigned *)(p + 2 * r4 + l4 + 2 * s8 + lk + lp);
    }
    return 2 * r4 + l4 + 2 * s8 + lk + lp + 256;
}

int rnnt_engine_ctc_workspace_bytes(int N, int T, int U, int V, size_t *out)
{
    if (!out) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument (out)");
    if (int rc = ctc_check_dims(N, T, U, V)) return rc;
    *out = ctc_carve(nullptr, N, T, U, nullptr);
    return RNNT_OK;
}

int rnnt_engine_ctc_loss_fwd_bwd(const void *logits, const int32_t *targets, const int32_t *logit_lens,
                                 const int32_t *target_lens, int N, int T, int U, int V, int blank,
                                 const float *cost_weights, float *costs, float *grad, void *ws, size_t ws_bytes, void *stream)
{
    if (int rc = ctc_check_dims(N, T, U, V)) return rc;
    if (!logits || !targets || !logit_lens || !target_lens || !costs || !ws) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    if (blank < 0 || blank >= V) return fail(RNNT_ERR_INVALID_ARG, "blank=%d outside [0,%d)", blank, V);
    if (!aligned16(logits) || (grad && !aligned16(grad)) || ((uintptr_t)ws & 255))
        return fail(RNNT_ERR_INVALID_ARG, "pointers must be 16-byte aligned (workspace 256)");
    const size_t need = ctc_carve(nullptr, N, T, U, nullptr);
    if (ws_bytes < need) return fail(RNNT_ERR_WORKSPACE, "workspace %zu < required %zu bytes", ws_bytes, need);
    CtcArgs a{};
    a.logits = (const float *)logits; a.targets = targets; a.logit_lens = logit_lens; a.target_lens = target_lens;
    a.weights = cost_weights; a.costs = costs; a.grad = grad;
    a.N = N; a.T = T; a.U = U; a.V = V; a.blank = blank;
    ctc_carve(ws, N, T, U, &a);
    launch_ctc_loss(a, (hipStream_t)stream);
    return launch_status("rnnt_engine_ctc_loss_fwd_bwd");
}

int rnnt_engine_ctc_greedy_decode(const void *logits, const int32_t *logit_lens, int N, int T, int V, int blank,
                                  int32_t *tokens, int32_t *counts, void *stream)
{
    if (int rc = ctc_check_dims(N, T, 0, V)) return rc;
    if (!logits || !logit_lens || !tokens || !counts) return fail(RNNT_ERR_INVALID_ARG, "null pointer argument");
    if (blank < 0 || blank >= V) return fail(RNNT_ERR_INVALID_ARG, "blank=%d outside [0,%d)", blank, V);
    if (!aligned16(logits)) return fail(RNNT_ERR_INVALID_ARG, "logits must be 16-byte aligned");
    launch_ctc_greedy((const float *)logits, logit_lens, N, T, V, blank, tokens, counts, (hipStream_t)stream);
    return launch_status("rnnt_engine_ctc_greedy_decode");
}

int rnnt_engine_run_stages(int stage_mask, int variant, const void *enc, const int64_t enc_strides[3],
                           const void *pred, const void *W, const void *bias, const int32_t *targets,
                           const int32_t *logit_lens, const int32_t *target_lens, int B, int T, int U1,
                           int H, int V, int blank, float clamp, float grad_scale, int dtype,
                           float *costs, void *grad_enc, void *grad_pred, void *grad_W,
                           void *grad_bias, void *workspace, size_t ws_bytes, void *stream)
{
    if (stage_mask <= 0 || stage_mask > ST_ALL) return fail(RNNT_ERR_INVALID_ARG, "stage_mask %d outside [1,255]", stage_mask);
    return run_fused(stage_mask, variant, enc, enc_strides, pred, W, bias, targets, logit_lens, target_lens,
                     B, T, U1, H, V, blank, clamp, grad_scale, 0.f, 0.f, dtype, costs, grad_enc, grad_pred, grad_W,
                     grad_bias, workspace, ws_bytes, stream);
}

int rnnt_engine_run_stage(int stage, const void *enc, const int64_t enc_strides[3],
                          const void *pred, const void *W, const void *bias,
                          const int32_t *targets, const int32_t *logit_lens,
                          const int32_t *target_lens, int B, int T, int U1, int H, int V, int blank,
                          float clamp, float grad_scale, int dtype, float *costs, void *grad_enc,
                          void *grad_pred, void *grad_W, void *grad_bias, void *workspace,
                          size_t ws_bytes, void *stream)
{
    if (stage < 0 || stage > 7) return fail(RNNT_ERR_INVALID_ARG, "stage %d outside [0,7]", stage);
    return run_fused(1 << stage, 0, enc, enc_strides, pred, W, bias, targets, logit_lens, target_lens,
                     B, T, U1, H, V, blank, clamp, grad_scale, 0.f, 0.f, dtype, costs, grad_enc, grad_pred,
                     grad_W, grad_bias, workspace, ws_bytes, stream);
}

}  // extern "C"
