// kernels.hpp — host-side launcher declarations shared by the engine's translation units.
#pragma once
#include "common.hpp"
#include "../../include/rnnt_engine.h"  // rnnt_conv_predictor_params (DecLoopArgs)

// ---- engine.hip: sets the thread-local error message, returns `code`
int engine_fail(int code, const char *fmt, ...);
// fills / copies as ordinary kernels on the caller's stream (in place of hipMemsetAsync / hipMemcpyAsync):
// a captured call is then a chain of kernel nodes only — with memset nodes in the chain, replays of a
// whole-pipeline HIP graph ran kernels against stale counters (ROCm 7.2; tests/test_gpu_parity.py::
// test_fused_call_is_hip_graph_capturable).  `bytes` and `p` multiples of 4.
void launch_fill32(void *p, unsigned value, size_t bytes, hipStream_t st);
void launch_copy_bytes(void *dst, const void *src, size_t bytes, hipStream_t st);
int device_cus();  // compute units of the current device, cached (x2.hip; the engine's and the Linear layers' persistent grids)

// ---- lattice.hip: the loss tail on the skewed work arrays (common.hpp), every stage on one argument block.  engine.hip fills it in
// one place per call (carve_loss_ws + the call's inputs and options); a launcher reads the fields its stage needs.
struct LatticeArgs {
    float *denom_s, *lpb_s, *lpe_s;   // skewed [B,D,U1]: log-sum-exp, lp_blank, lp_emit of every lattice cell (the producers' output)
    double *alpha_s, *beta_s;         // skewed [B,D,U1] fp64
    CellCoef *coef;                   // [B,T,U1]
    unsigned *err;                    // one word: raised by a chained sweep whose bounded spin ran out
    const int32_t *targets, *logit_lens, *target_lens;  // [B,U1-1], [B], [B]
    float *costs;                     // [B]
    int B, T, U1, D;                  // D = T + U1 - 1 diagonals
    float grad_scale;                 // the coefficients are those of grad_scale * sum_b costs[b]
    float fastemit, delay;            // FastEmit's lambda and the delay penalty's delta; 0: off
    const int32_t *restrict_frames;   // [B,U1-1] alignment restriction, or null: none
    int restrict_left, restrict_right;
    bool flush;                       // the f16x2 route's flush rule (lattice.hip k_coef, FLUSH) with the two thresholds below;
    double flush_log2; float flush_lin;  // flush_log2 = -inf, flush_lin = 0 flag nothing
    int V, blank;                     // the vocabulary (V % 4 == 0) and the blank's index
    // the entries on materialised logits only (launch_logsoftmax_gather, launch_grad_logits), else null / 0:
    const float *logits; float *grad_logits; float clamp;  // [B,T,U1,V]; clamp > 0 bounds every entry of grad_logits
};
void launch_logsoftmax_gather(const LatticeArgs &a, hipStream_t st);  // logits -> denom_s, lpb_s, lpe_s
// The stages in call order (engine.hip loss_stages).  launch_lp_emit: the pass over lp_emit before the sweep — label arcs outside
// their window get -inf (restrict_frames), the others the delay penalty; a call with neither does not run it.  launch_lattice:
// alpha_s, beta_s, costs (the -inf-safe chained sweep on a restricted lattice).  launch_delay_cost: the cost the penalty shifted, put
// back (delay > 0 only).  launch_coef: the coefficients — FastEmit's when fastemit > 0, else the flush rule's when `flush`, else the
// plain ones; on a restricted lattice with dead cells (alpha or beta = -inf, cost = +inf) set to those of a cell outside the lattice.
void launch_lp_emit(const LatticeArgs &a, hipStream_t st);
void launch_lattice(const LatticeArgs &a, hipStream_t st);
void launch_delay_cost(const LatticeArgs &a, hipStream_t st);
void launch_coef(const LatticeArgs &a, hipStream_t st);
void launch_grad_logits(const LatticeArgs &a, hipStream_t st);  // coef, logits -> grad_logits
// a chained sweep's failure report (lattice.hip's and ctc.hip's): *err != 0 turns costs[0..n) — and logp[0..n), unless null — into NaN
void launch_chain_status(const unsigned *err, float *costs, double *logp, int n, hipStream_t st);

// ---- align.hip: forced alignment on the lp arrays of either producer (lpb_s, lpe_s, the lengths and the
// dimensions of `a`).  `bp`: the backpointer words, B * D * ceil(U1/64) u64 (fits in the alpha_s region of both workspaces);
// frames [B, U1-1] int32; scores [B].
void launch_align(const LatticeArgs &a, void *bp, float *scores, int32_t *frames, hipStream_t st);

// ---- joint_fwd.hip
struct JointFwdArgs {
    const float *enc;   // [B,T,H], h-stride 1
    long enc_sb, enc_st;
    const float *pred;  // [B,U1,H] contiguous
    const float *wpack; // packed W (pack_w_fwd)
    const float *hidden; // [rows,H] tanh(enc+pred) (fused path), else NULL
    int make_hidden;     // 1: the forward kernel itself fills `hidden` for its tile (no k_make_hidden pass)
    const float *bias;  // [V]
    const int32_t *targets, *logit_lens, *target_lens;  // all NULL for the plain joint
    float *logits;      // [B,T,U1,V]
    float *denom_s, *lpb_s, *lpe_s;  // skewed [B,D,U1]; NULL for the plain joint
    int B, T, U1, H, V, D, blank;
    int ablate;  // diagnostic builds: the ablation word of rnnt_engine_set_flags, read through RNNT_XP only (bit0: non-temporal logits stores); never anything else
    unsigned *counter;  // one zeroable word: tile counter of the persistent forward (NULL: one workgroup per tile)
    int n_cu;           // compute units
    unsigned long long *debug;  // diagnostic stamp buffer (RNNT_STAMPS builds), else NULL
};
size_t wpack_floats(int H, int V);
void launch_pack_w_fwd(const float *W, float *wpack, int H, int V, hipStream_t st);
// lds_ring: W through an LDS-DMA ring (RNNT_VARIANT_FWD_LDS_RING); one_wg_per_tile: no persistent workgroups (RNNT_VARIANT_FWD_ONE_WG_PER_TILE)
void launch_joint_fwd(const JointFwdArgs &a, hipStream_t st, bool lds_ring = false, bool one_wg_per_tile = false);
int fwd_occupancy(int with_loss);
void launch_zero_dead_hidden(float *hidden, const int32_t *logit_lens, const int32_t *target_lens, int B, int T,
                             int U1, int H, hipStream_t st);
void launch_copy_enc(const float *enc, long sb, long st_, long sh, float *dst, int B, int T, int H,
                     hipStream_t st);

// ---- joint_bwd.hip
struct JointBwdArgs {
    const float *enc; long enc_sb, enc_st;
    const float *pred;
    const float *W;       // [V,H] natural layout
    const float *logits;  // [rows_pad,V]: logits, overwritten by G (k_make_g)
    float *hidden;        // [rows_pad,H] tanh(enc+pred) (k_make_hidden)
    long rows_pad;        // B*T*U1 rounded up to a multiple of 16 (zero rows)
    const CellCoef *coef; // [B,T,U1]
    const int32_t *logit_lens, *target_lens;
    float *slab_enc;   // [n_ublk][B,T,H]
    float *slab_pred;  // [n_ttile][B,U1,H]
    float *slab_w;     // [n_split][V,H]
    float *slab_b;     // [n_split][V]
    float *grad_enc, *grad_pred, *grad_W, *grad_bias;
    int B, T, U1, H, V, blank;
    int n_ublk, n_ttile, n_split;
    unsigned *counter;  // 8 x 64 zeroed bytes: per-XCD work-item counters of the persistent kernels
    long *dw_tab;       // dW live-granule region (launch_dw_list): [0] live count, block offsets, list
    const int *dw_list; // set by launch_dw: the list inside that region
    int n_cu;           // compute units (grid size of the persistent kernels)
    int ablate;         // diagnostic builds: the ablation word of rnnt_engine_set_flags (RNNT_XP), nothing else
    int g_ready;        // on the tile kernel (launch_dhidden): G already stands in place of the logits (k_make_g ran): the first column group reads it too (GEN = false)
    int gen_bu;         // u width of k_dhidden_gen's tiles (16, or 8 for short targets); dEnc slabs of columns < pred_split_col
    int pred_split_col; // dPred slabs: columns < this come in 8-row t tiles (k_dhidden_gen, bf16 route), the rest in 4-row tiles (k_dhidden)
    // f16x2 route only (x2.hip "flush rule"), NULL on every other: the reductions add a slab piece only where its 8 t x 16 u tile's flag is 1
    // (dead tiles write no slab); [B][flag_ntt][flag_nub]
    const unsigned char *tile_flag;
    int flag_ntt, flag_nub;
    unsigned long long *debug;  // diagnostic stamp buffer (RNNT_STAMPS builds), else NULL
};
// tile_kernel: k_dhidden_gen on the whole 512-column groups (the caller decides: dhidden_gen_ok), producing G unless g_ready; the persistent k_dhidden on the rest
void launch_dhidden(const JointBwdArgs &a, bool tile_kernel, hipStream_t st);
void launch_dw(const JointBwdArgs &a, hipStream_t st);
int dw_tiles(int H, int V);  // workgroup tiles per split of k_dw
void launch_dw_table(const int32_t *logit_lens, int B, int T, int U1, int gran, long *tab, hipStream_t st);
// the dW GEMMs of the MFMA routes (split_dw.hpp): cells per granule of their live-row table; rows their DMA rings may read past rows_pad
// (zero padding rows, bf16_rows_alloc: k_dw_bf16 three stages of 32, k_dw_x3 two k-steps of 16, k_dw_x2 none past its lists' padding
// entries) — each kernel asserts its read-ahead against it
#define DW_GRAN 32
#define DW_ROWS_PAST 96
size_t dw_list_bytes(int B, int T, int U1, int gran);  // bytes of the live-granule region of launch_dw
void launch_dhidden_reduce(const JointBwdArgs &a, hipStream_t st);
void launch_dw_reduce(const JointBwdArgs &a, hipStream_t st);
void launch_make_hidden(const JointBwdArgs &a, hipStream_t st);
void launch_make_g(const JointBwdArgs &a, hipStream_t st);
bool dhidden_gen_ok(int H, int V, int U1);
int dhidden_gen_groups(int H);  // 512-column groups on the tile kernel (the rest: persistent k_dhidden)
int dhidden_gen_bu(int T, int U1);  // 16 or 8: the tile form that pads the lattice least  // k_dhidden_gen (G produced inside the dHidden GEMM) applies

// ---- bf16.hip (RNNT_DTYPE_BF16 route: bf16 GEMM operands, fp32 accumulate / logits / loss)
struct Bf16Args {
    const float *enc; long enc_sb, enc_st;
    const float *pred;
    const float *W;      // [V,H] fp32 (re-packed to bf16 fragment order every call)
    const float *bias;
    unsigned short *hidden;  // bf16 [rows_alloc,H] tanh(enc+pred)
    void *wpack_fwd, *wpack_dh;
    unsigned short *logits;  // fp16 [rows_alloc,V]; G (bf16) overwrites each row in place
    const CellCoef *coef;
    const int32_t *targets, *logit_lens, *target_lens;
    float *denom_s, *lpb_s, *lpe_s;  // skewed [B,D,U1] softmax statistics (forward epilogue)
    int D;
    float *slab_enc, *slab_pred, *slab_w, *slab_b;
    long rows_alloc;     // multiple of 128, >= rows_pad + 96; rows >= B*T*U1 are zero
    long rows_pad;       // K extent of the dW GEMM (multiple of 32)
    int B, T, U1, H, V, blank;
    int n_ublk, n_split;
    int ablate;  // diagnostic builds: the ablation word of rnnt_engine_set_flags (RNNT_XP; bits 8..: 256 no stores, 512 no statistics, 1024 no MFMA), nothing else
    long *dw_tab;  // 2B+2 longs: live-row table of k_dw_bf16 (k_dw_table at DW_GRAN cells per granule; walked as split_dw.hpp's DwShare)
    unsigned long long *debug;  // diagnostic stamp buffer (RNNT_STAMPS builds), else NULL
    int *dw_prog;  // [n_split][16] progress words of the soft lockstep of k_dw_bf16's tiles: stages done over all ranges, 0x7fffffff at the end (zeroed by its launcher), or NULL
};
size_t bf16_wpack_fwd_bytes(int H, int V);
size_t bf16_wpack_dh_bytes(int H, int V);
void launch_bf16_producers(const Bf16Args &a, hipStream_t st);
void launch_joint_fwd_bf16(const Bf16Args &a, hipStream_t st);
void launch_dhidden_bf16(const Bf16Args &a, hipStream_t st);
void launch_dw_bf16(const Bf16Args &a, hipStream_t st);

// ---- x3.hip (RNNT_DTYPE_F32_BF16X3 route: fp32-accurate products as six bf16 MFMA products of 3-way split operands)
struct X3Args {
    const float *enc; long enc_sb, enc_st;
    const float *pred;
    const float *W;      // [V,H] fp32 (split and re-packed in fragment order every call)
    const float *bias;
    unsigned short *hidden;  // bf16 planes [3][rows_alloc][H] of tanh(enc+pred): hi, mid, lo
    long plane_stride;       // elements between two planes of `hidden` (= rows_alloc * H)
    void *wpack_fwd, *wpack_dh;
    float *logits;           // fp32 [rows_alloc,V]; G's hi | mid planes overwrite each 32-wide chunk in place
    unsigned short *g_lo;    // bf16 [rows_alloc,V]: lo plane of G
    const CellCoef *coef;
    const int32_t *targets, *logit_lens, *target_lens;
    float *denom_s, *lpb_s, *lpe_s;  // skewed [B,D,U1] softmax statistics (forward epilogue)
    int D;
    float *slab_enc, *slab_pred, *slab_w, *slab_b;
    long rows_alloc;     // multiple of 128, >= rows_pad + 96; rows >= B*T*U1 are zero
    long rows_pad;       // K extent of the dW GEMM (multiple of 32)
    int B, T, U1, H, V, blank;
    int n_ublk, n_split;
    int n_ublk16;        // u blocks of k_dhidden_x3 (16 wide)
    int ablate;          // diagnostic builds: the ablation word of rnnt_engine_set_flags (RNNT_XP), nothing else
    long *dw_tab;        // 2B+2 longs: live-row table of k_dw_x3 (k_dw_table at DW_GRAN cells per granule; split_dw.hpp: DwShare, dw_walk_ranges)
    unsigned *counter;   // zeroable word: tile counter of the persistent forward
    int n_cu;
    unsigned long long *debug;  // diagnostic stamp buffer (RNNT_STAMPS builds), else NULL
    // RNNT_DTYPE_F32_F16X2 (x2.hip; `hidden` then holds two fp16 planes, G two fp16 planes in place of the logits, no g_lo):
    float g_scale;              // power of two with |g_scale G| <= 2^13 (from grad_scale)
    float dw_rescale, db_rescale;  // 1 / (g_scale 2^14), 1 / g_scale
    const float *scales;        // device: {s_W, 1 / s_W} (k_x2_wscale, every call)
    int *dw_prog;               // [n_split][16] progress words of k_dw_x2's / k_dw_x2m's tiles (split_dw.hpp: DwLockstep; k-steps of the pipeline run; zeroed by the launcher), or NULL
    float *ep_enc, *ep_pred;    // exp(2 enc) [B][H/16][T][16], exp(2 pred) [B][H/16][U1][16] (k_x2_make_ep, every call)
    unsigned *ep_flag;          // device word: != 0 when an input lies outside the factored tanh's range (the exact forward runs)
    // live structures of the backward (launch_x2_live, after the coefficients; x2.hip "flush rule"); the Linear layer's dW sets ks_list / grp_list / live_stats only
    const unsigned char *tile_live;  // [B][ceil(T/8)][n_ublk16]: 1 = the dHidden tile holds a cell with non-null coefficients
    const unsigned *ks_bitmap;       // bit k: 16-cell k-step k of the dW GEMM is live (holds such a cell); what k_dw_x2m walks as ks_list
    int *ks_list;                    // ascending live k-steps, then >= 8 entries naming the first all-padding k-step (rows_pad / 16)
    const unsigned *grp_bitmap;      // bit g: cells 4g .. 4g+3 (linear cell order) hold a live cell; what k_dw_x2 walks as grp_list
    int *grp_list;                   // ascending live groups, 16-byte aligned, then >= 4 ring stages + 3 entries naming the first all-padding group (rows_pad / 4)
    int *live_stats;                 // [0] live k-steps = length of ks_list, [1] k-steps with a cell, [2] live dHidden tiles = length of tile_list, [3] dHidden tiles,
                                     // [4] live groups = length of grp_list, [5] groups with a cell
    const int *tile_list;            // ascending indices [b][tt][ub] of the tiles whose flag is 1: the workgroups of k_dhidden_x2 (entries past live_stats[2] hold anything)
    int dw_ksteps;                   // 1: the dW kernel of this call walks ks_list (k_dw_x2m): k_x2_dead_rows zeroes the dead tiles' rows of the live k-steps, not of the live groups
};
size_t x2_live_bytes(int B, int T, int U1, long rows_pad);  // bytes of the region below
void x2_live_carve(void *region, int B, int T, int U1, long rows_pad, X3Args &a);  // points tile_live .. grp_list into the region
void launch_x2_live(const X3Args &a, hipStream_t st);  // builds them all from X3Args::coef
// the split routes' forward kernels (k_joint_fwd_x3, k_joint_fwd_x2) cover this shape (else: the fp32 route's)
inline bool split_fwd_ok(int U1, int H, int V) { return H % 128 == 0 && V % 128 == 0 && (long)128 * H * 2 < 0x7fffffffL; }
bool x3_dhidden_ok(int U1, int H, int V);  // likewise k_dhidden_x3
size_t x3_wpack_fwd_bytes(int H, int V);
size_t x3_wpack_dh_bytes(int H, int V);
void launch_x3_make_hidden(const X3Args &a, hipStream_t st);
void launch_x3_split_g(const X3Args &a, hipStream_t st);
void launch_x3_zero_padding(const X3Args &a, int what, hipStream_t st);
void launch_x3_pack_w(const X3Args &a, hipStream_t st);
void launch_joint_fwd_x3(const X3Args &a, hipStream_t st);   // one 512-register wave per SIMD (default)
void launch_dhidden_x3(const X3Args &a, hipStream_t st);
void launch_dw_x3(const X3Args &a, hipStream_t st);   // v_mfma_f32_32x32x16_bf16, six products per k-step (default)
// RNNT_DTYPE_F32_F16X2 (x2.hip): the bf16x3 route's stages on two fp16 planes and three products
bool x2_dhidden_ok(int U1, int H, int V);
size_t x2_wpack_fwd_bytes(int H, int V);
size_t x2_wpack_dh_bytes(int H, int V);
void launch_x2_make_hidden(const X3Args &a, hipStream_t st);
void launch_x2_split_g(const X3Args &a, hipStream_t st);
void launch_x2_zero_padding(const X3Args &a, int what, hipStream_t st);
void launch_x2_pack_w(const X3Args &a, float *scales, hipStream_t st);  // s_W from max |W|, then both packs
void launch_x2_make_ep(const X3Args &a, hipStream_t st);               // exp(2 enc), exp(2 pred) in k-step-major layout + the range flag
size_t x2_ep_bytes(int B, int T, int U1, int H);
void launch_joint_fwd_x2(const X3Args &a, hipStream_t st, bool plain_gemm = false);   // one 512-register wave per SIMD; plain_gemm: k_joint_fwd_x2<2> (the Linear layers)
void launch_x2_dead_rows(const X3Args &a, hipStream_t st);  // zero G rows of dead tiles' cells inside live groups (what k_dw_x2 reads beside the live tiles' rows; X3Args::dw_ksteps: inside live k-steps)
void launch_dhidden_x2(const X3Args &a, hipStream_t st);
// the joint's input projections (audio_ln / text_ln) and their backward on the f16x2 pipes (x2.hip, round 5)
size_t x2_linear_ws_bytes(int M, int K, int N, bool bwd);
bool x2_linear_ok(int M, int K, int N);
void launch_linear_x2_fwd(const float *x, long ldx, const float *W, const float *bias, int M, int K, int N, float *y, void *ws, hipStream_t st);
void launch_linear_x2_bwd(const float *x, long ldx, const float *W, const float *dy, int M, int K, int N, float *dx, float *dW, float *db, void *ws,
                          hipStream_t st);
int x2_dw_tiles(int H, int V);  // workgroup tiles per split of launch_dw_x2 (k_dw_x2 / k_dw_x2m)
void launch_dw_reduce_x2(const X3Args &a, float *grad_W, float *grad_bias, hipStream_t st);  // the slabs' sum, fp64 accumulate, one rounding
bool x2_dw_walks_ksteps(int H, int V);  // launch_dw_x2's kernel for this shape reads X3Args::ks_list (k_dw_x2m), not X3Args::grp_list
void launch_dw_x2(const X3Args &a, hipStream_t st, bool zero_prog = true);  // k_dw_x2<4> (k_dw_x2<4, true> when H % 256 == 128), k_dw_x2m where x2_dw_mixed_ok

// ---- decode.hip
void launch_scan_logits(const float *enc, long enc_st, const float *pred, const float *W, const float *bias,
                        float *logits, int K, int H, int V, hipStream_t st);
void launch_argmax_scan(const float *logits, int K, int V, int blank, int t0, int32_t *out, hipStream_t st);

// device-resident greedy decode (decode.hip)
struct DecLoopArgs {
    const float *frames; long frame_stride; int T;  // [T,H] audio frames (after audio_ln), h-stride 1
    rnnt_conv_predictor_params p; int S, E, O; float ln_in_eps, ln_eps;  // eps of input_layer_norm / output_layer_norm
    const float *text_W, *text_b;                   // joint.text_ln [H,O], [H] or NULL (then O == H)
    const float *W, *bias; int H, V, blank;         // joint_ln
    int max_length, max_per_frame, scan_frames, iterations;
    int init;              // 1: initialise state, rings and weight packs first; 0: continue a decode in progress
    int32_t *host_flag;    // device pointer of a mapped host word set to 1 when the loop ends, or NULL
    int32_t *state, *tokens;
    void *workspace;
    const void *tables = nullptr;  // launch_dec_persist: the model's tables (launch_dec_build_tables), or NULL: built in the workspace
    const int32_t *sstate = nullptr;  // a stream's push (launch_dec_stream): the canonical state block, read; NULL: a whole utterance
    int stream_cap = 0;               // a stream's push: labels it may emit at most (max_length then 0 = unbounded)
};
size_t dec_loop_workspace_floats(int H, int V, int E, int O, int nframes);
void launch_dec_loop(const DecLoopArgs &a, hipStream_t st);
// the same loop as ONE persistent launch (decode.hip, k_dec_persist): granule buffers, tables and folded matrices live in the workspace
struct DecPersistArgs {
    unsigned long long *g2g, *zg, *sg, *cg;         // hand-off granules: g2 [E] | z or q [H] | z's (mean, M2) per workgroup | candidates [2][16][G]
    const float *Eenc; int T;                        // exp(2 frames) [T,H]
    const float *A0, *A1, *A2, *conv1_b;             // conv1 as tables: tap j's row of symbol s at A_j + 3 E s
    const float *wp2, *conv2_b;                      // conv2 pack [5][E][E]
    const float *Wl, *bl;                            // linear [O,E], [O]
    const float *M, *dvec, *rvec, *cvec;             // with text_ln: M [H,E], d, r, c [H]
    const float *gamma, *beta; float eps;            // output LayerNorm
    const float *W, *bias;                           // joint_ln [V,H], [V]
    int S, E, O, H, V, blank, max_length, max_per_frame, has_text, max_iters;
    int32_t *state, *tokens, *host_flag;
    const int32_t *sstate;                           // a stream's push: resume from this state block, else NULL
    int tok0, lds_toks;                              // label i (1-based) goes to tokens[tok0 + i - 1]; collected in LDS first (<= DP_TOKS - 1 labels)
};
int dec_persist_groups(int V);
const char *dec_persist_refusal(int T, int S, int E, int O, int H, int V, int has_text);  // NULL: supported
size_t dec_persist_workspace_floats(int T, int S, int E, int O, int H, int V, int has_text);
size_t dec_persist_lds_bytes(int E);
int launch_dec_persist(const DecLoopArgs &a, hipStream_t st);  // hipSuccess, or why the kernel's LDS limit could not be raised (nothing launched);  // scan_frames / iterations / init of `a` are not used
size_t dec_tables_floats(int S, int E, int O, int H, int has_text);
void launch_dec_build_tables(const rnnt_conv_predictor_params &p, int S, int E, int O, float ln_in_eps, const float *text_W, const float *text_b, int H,
                             float *tables, hipStream_t st);
// offsets (floats) of the conv1 tap tables tab[s][tap][E] and of conv2's [tap][out][in] pack inside those tables
void dec_tables_offsets(int S, int E, int O, int H, int has_text, size_t *tab, size_t *wp2);
// streaming greedy decode (decode.hip): one push of a.T >= 0 frames from the state block a.sstate (rnnt_engine_greedy_stream_decode)
void launch_stream_init(int32_t *state, int blank, hipStream_t st);
size_t dec_stream_workspace_bytes(int n, int S, int E, int O, int H, int V, int has_text, int cap, int persistent);
int launch_dec_stream(const DecLoopArgs &a, int persistent, hipStream_t st);  // hipSuccess, or the persistent kernel's LDS-limit error (nothing launched)

// ---- beam.hip: frame-synchronous beam search (rnnt_engine_beam_decode: one utterance; rnnt_engine_beam_decode_batch: n_utt in lockstep;
// rnnt_engine_beam_stream_push: n_streams searches resting between pushes), kernel-per-step rounds
struct BeamArgs {
    DecLoopArgs d;       // frames, predictor, joint, blank, max_length, max_per_frame, iterations (= rounds), init, host_flag, state, tokens
    int beam;            // 1 .. 16
    double *scores;      // [beam] out ([n_utt][beam])
    // the batched search (else utt == NULL): d.frames holds `rows` packed rows, d.state is [n_utt][32], d.tokens [n_utt][beam][max_length]
    const int32_t *utt = nullptr;  // device int32[n_utt][2]: each utterance's first row and frame count
    int n_utt = 1, rows = 0;
    // a push of n_utt streams (rnnt_engine_beam_stream_push): utt is the push's table, d.workspace the streams' persistent block (its layout:
    // beam_stream_block_bytes), d.tables required, d.init = open the push (k_beam_stream_begin) before the rounds
    bool streaming = false;
    // contextual biasing (rnnt_engine_beam_decode_ctx / _batch_ctx; never with streaming): the caller's graph, its arrays on the device;
    // the workspace is then the one of beam_workspace_bytes(..., ctx = true) (a node per slot more)
    const rnnt_beam_context *ctx = nullptr;
};
size_t beam_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, bool ctx = false);
size_t beam_batch_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int n_utt, bool ctx = false);
void launch_beam_decode(const BeamArgs &a, hipStream_t st);
size_t beam_stream_block_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int n_streams);
void launch_beam_stream_init(void *block, int32_t *state, double *scores, int S, int E, int O, int H, int V, int has_text, int max_length,
                             int beam, int blank, int n_streams, int first, int count, hipStream_t st);

// ---- beam search with the LSTMPredictor (rnnt_engine_beam_decode_lstm; DESIGN.md §4h "LSTM"): the batched search of beam.hip whose predictor
// step is lstm.hip's.  Row 16 u + s of every product is slot s of utterance u.
enum { BEAM_ST_DONE = 3, BEAM_ST_NEW = 4, BEAM_ST_CUR = 6 };  // the words of a search's state the predictor step reads (beam.hip: BS_*)
struct BeamLstmStep {
    // the searches, as beam.hip lays them out: utterance u's copy of a per-search array lies u * stride BYTES after utterance 0's
    const int32_t *state;          // [n_utt][32]
    const int *need, *len, *tok;   // [2][16] | [2][16] | [2][16][max_length]
    float *pvec;                   // [2][16][H]: the step's result goes to the slot's row of the CURRENT buffer
    size_t stride; int n_utt, max_length;
    // LSTM state: `pool` [32 n_utt][L][2][Hd]; slot 16 u + s continues the state in row par[16 u + s] and owns row own[16 u + s]
    const int *own, *par; float *pool;
    rnnt_lstm_predictor_params p; int S, E, Hd, O, L, ln; float eps_in, eps_lstm, eps_out;
    const float *text_W, *text_b; int H;  // joint.text_ln or NULL (then O == H)
    float *scratch;                       // beam_lstm_step_floats(...) floats; no value in it outlives a round
};
size_t beam_lstm_step_floats(int n_utt, int E, int Hd, int O, int H);
void launch_beam_lstm_step(const BeamLstmStep &a, hipStream_t st);  // lstm.hip: the predictor step of one round, 3 + 2 L launches (2 more with text_ln)
struct BeamLstmArgs {
    BeamLstmStep s;  // the model; state .. pool and scratch are filled in by launch_beam_decode_lstm
    const float *frames; long frame_stride; int rows; const int32_t *utt;
    const float *W, *bias; int V, blank, max_per_frame, beam, iterations, init;
    int32_t *host_flag, *state, *tokens; double *scores; void *workspace;
};
size_t beam_lstm_workspace_bytes(int n_utt, int E, int Hd, int O, int L, int H, int V, int max_length);
void launch_beam_decode_lstm(const BeamLstmArgs &a, hipStream_t st);  // beam.hip

// ---- ctc.hip: the CTC auxiliary head.  Arrays of the loss, all in the caller's workspace: denom / lpb [N,T], lpl [N,T,max(U,1)],
// alpha / beta [N,T,2(U+1)] fp64 by lattice state (2u: the blank before label u, 2u+1: label u), link [N,max(U,1)], logp [N] fp64, err one word.
struct CtcArgs {
    const float *logits;                                // [N,T,V], V % 4 == 0
    const int32_t *targets, *logit_lens, *target_lens;  // [N,U], [N], [N]
    const float *weights;                               // [N] or NULL (= 1): d (weight_n cost_n) / d logits
    float *costs, *grad;                                // [N]; [N,T,V] or NULL (costs only)
    float *denom, *lpb, *lpl; double *alpha, *beta; int32_t *link; double *logp; unsigned *err;
    int N, T, U, V, blank;                              // U <= 1023
};
void launch_ctc_loss(const CtcArgs &a, hipStream_t st);
void launch_ctc_greedy(const float *logits, const int32_t *logit_lens, int N, int T, int V, int blank, int32_t *tokens,
                       int32_t *counts, hipStream_t st);
