// beam.hip — frame-synchronous beam search on the device: ONE utterance (rnnt_engine_beam_decode), N independent ones advanced in
// lockstep by the same rounds (rnnt_engine_beam_decode_batch), or N STREAMS whose searches rest at the end of every push of frames and
// resume at the next (rnnt_engine_beam_stream_push); DESIGN.md §4h, §4l.
//
// The search (exact definition: DESIGN.md §4h, tests/beam_oracle.py): at most `m` labels per frame, hypotheses merged by
// token sequence; beam 1 is the reference's greedy decode (rnnt/model.py:95-128).  Per frame t, rounds r = 0 .. m-1: every
// ACTIVE hypothesis h is scored lp = log_softmax(single_forward(frame_t, predictor([blank] + y_h)[-1])); its blank candidate
// (y_h, score + lp[blank]) joins the finished set N of the frame (merged by sequence with logaddexp), its label candidates
// (y_h + [k], score + lp[k]), k != blank, are generated while len(y_h) < max_length - 1; the best `beam` of N + labels are
// kept, the kept labels are the next round's actives.  The frame ends when no label is kept; after round m-1 kept labels
// are CAPPED: they move to the next frame without a blank term, merged with N by sequence.
//
// One ROUND is a fixed kernel sequence over the <= 16 slots of the beam — the slots are the M = 16 rows of every product:
//   k_beam_conv1   conv1 outputs of the last 5 positions of every slot that just took a label, from the tap tables of
//                  rnnt_engine_greedy_decode_build_tables (A_j[s] = W1_j LN(embedding[s])): the conv1-output ring, rebuilt
//                  from the slot's last 7 tokens (the module is causal: its last frame is a function of those only)
//   k_beam_gemm16  conv2 (5 taps, GELU), linear, with joint.text_ln the projection of LN(z): 16 rows x 16 outputs per
//                  workgroup on v_mfma_f32_16x16x4_f32, every weight read once per round for all slots
//   k_beam_ln16    (no text_ln) the predictor's output LayerNorm -> the slot's text vector
//   k_beam_joint   logits [16][V] = tanh(frame_t + text_slot) W^T + bias: vocabulary-parallel, 16 entries per workgroup,
//                  tanh of the SUM (no factored form, no range limit)
//   k_beam_reduce  per active slot: log-sum-exp, the blank logit and the top-`beam` non-blank labels
//   k_beam_select  one workgroup: candidates, merges by sequence (64-bit hash as a pre-filter, exact comparison), the best
//                  `beam`, the cap, max_length, t / round / done, the next slot buffer (tokens, lengths, scores, text vectors)
// The predictor kernels return at once in rounds where no slot took a label (round 0 of a frame after a blank-only one),
// every kernel once the search is over.  Nothing spins; no workgroup waits for another.
// The batched search: every kernel is a template over a trailing argument pack `U... ub` — EMPTY for the single search, whose
// instantiation has exactly the arguments and the body it had before there was a batch (u = 0 and a zero stride fold away), one
// BeamBatch for the batched search, where the utterance is grid.y.  Everything a search owns — its slot buffers, intermediates,
// logits, state, results — lies `stride` bytes (its own size) after its neighbour's, the weights and tables are shared, and a
// workgroup of utterance u does exactly what the single search's workgroup does, on u's block.  A done search's workgroups return
// at once; the last one to finish raises the host's flag (a device-scope counter, k_beam_select).
// The streaming search: a third pack, one BeamStream — the batch's layout and grid, with the caller's persistent block in
// the workspace's place.  A stream never ends: the search that completes the last frame of its push writes its result as a search that
// ends does and sets its AT-REST word, which is what its kernels test where the other two test `done`; k_beam_stream_begin opens the
// next push (the frames consumed so far become the base of the push's row addressing, the word is cleared).
// Contextual biasing (DESIGN.md §4h "Context"; rnnt_engine_beam_decode_ctx / _batch_ctx): a BeamCtx — the caller's phrase list as an
// Aho–Corasick trie in flat device arrays, and a node per slot — as the LAST member of the pack of k_beam_reduce and k_beam_select only:
// the reduce re-ranks a slot's labels by logit + delta(node, label) in a tail of its wave 0, the selection adds the delta in fp64 and
// moves the nodes with the hypotheses.  The packs <> and <BeamBatch> are the instantiations they were; a stream takes no graph.
// The search with the LSTMPredictor (DESIGN.md §4h "LSTM"; rnnt_engine_beam_decode_lstm, at the end of the file): the batched search whose
// predictor step is lstm.hip's and whose selection takes a BeamLstm as the pack's last member — it moves a hypothesis's LSTM state as an index.
// Arithmetic: fp32 products (fp32 MFMA, exact fp32 as fmaf chains), log-sum-exp in fp32, SCORES in fp64 (the log-probability
// (double)logit - (double)lse is added to a double score; logaddexp in double).
// Ties (no result may depend on one): finished entries first, then parent slot ascending, then token id ascending; the
// per-slot top labels break ties by the lower token id (torch.argmax's first index at beam 1).
#include "decode_kernels.hpp"
#include <type_traits>

#define BM 16          // slots: the M dimension of every product
#define BEAM_RED 48    // floats per slot of k_beam_reduce's output: [0] lse, [1] blank logit, [16 + 2q] q-th label logit, [17 + 2q] its id
#define BEAM_NC (32 + BM * BM)  // candidates of one selection: <= 32 finished, beam x beam labels
#define BEAM_HASH_MUL 0x100000001b3ULL

// state (int32[32]) — also the caller's view of the search:
//   [0] t  [1] round within the frame  [2] entries of the beam  [3] done  [4] some slot awaits its predictor step
//   [5] rounds that did work  [6] current slot buffer (0 / 1)  [8 + j] length of entry j of the result (done)
//   a stream (RNNT_BEAM_STREAM_* of include/rnnt_engine.h): [0] counts the frames consumed over all pushes, [3] stays 0,
//   [24] at rest: every frame pushed so far is consumed  [25] frames consumed when the current push began
enum { BS_T = 0, BS_R = 1, BS_N = 2, BS_DONE = 3, BS_NEW = 4, BS_ROUNDS = 5, BS_CUR = 6, BS_LEN = 8,
       BS_REST = RNNT_BEAM_STREAM_AT_REST, BS_BASE = RNNT_BEAM_STREAM_BASE };
static_assert(RNNT_BEAM_STREAM_FRAMES == BS_T && BS_REST >= BS_LEN + BM && BS_BASE >= BS_LEN + BM && BS_REST != BS_BASE && BS_REST < 32 &&
              BS_BASE < 32, "the stream's words lie in the free part of the state");
// slot status
enum { SL_EMPTY = 0, SL_ACTIVE = 1, SL_FINISHED = 2 };

// ---- contextual biasing (DESIGN.md §4h "Context"): the phrase list as an Aho–Corasick trie in flat device arrays, one node per slot.
// The tables are the caller's device memory and are NOT trusted: every node index read from them is clamped to [0, n_nodes), every
// child range to [0, n_children], depths to [0, BEAM_CTX_DEPTH], the fail walk is a counted loop of BEAM_CTX_DEPTH hops and the child
// search a counted bisection — a malformed table gives a wrong result, never an access out of range or a loop without end.
#define BEAM_CTX_DEPTH 64
struct BeamCtx {
    const int32_t *child_off;   // [n_nodes + 1]: node m's children are entries child_off[m] .. child_off[m + 1] - 1
    const int32_t *child_tok;   // [n_children]: their tokens, ascending within a node
    const int32_t *child_node;  // [n_children]: the nodes they lead to
    const int32_t *fail;        // [n_nodes]: the deepest proper suffix of the node's path that is a path of the trie
    const int32_t *depth;       // [n_nodes]: bonus(n) = score * depth(n)
    const int32_t *terminal;    // [n_nodes]: a phrase ends here (the next state is the root: its bonus is banked)
    int n_nodes, n_children;
    double score;
    int *node;                  // [2][BM] the slots' nodes (workspace; double-buffered like len and hash)
};
struct BeamStep { int next, ddepth; };  // the next node | depth(m') - depth(n)
__device__ __forceinline__ int beam_ctx_node(const BeamCtx &c, int n) { return n < 0 ? 0 : (n >= c.n_nodes ? c.n_nodes - 1 : n); }
__device__ __forceinline__ int beam_ctx_depth(const BeamCtx &c, int n) { const int d = c.depth[n]; return d < 0 ? 0 : (d > BEAM_CTX_DEPTH ? BEAM_CTX_DEPTH : d); }
__device__ __forceinline__ void beam_ctx_range(const BeamCtx &c, int m, int &lo, int &hi)
{
    lo = c.child_off[m]; hi = c.child_off[m + 1];
    lo = lo < 0 ? 0 : (lo > c.n_children ? c.n_children : lo);
    hi = hi < lo ? lo : (hi > c.n_children ? c.n_children : hi);
}
// the child of node m (already clamped) by token k: its index in the child arrays, or -1
__device__ __forceinline__ int beam_ctx_child(const BeamCtx &c, int m, int k)
{
    int lo, hi;
    beam_ctx_range(c, m, lo, hi);
    for (int it = 0; it < 32 && lo < hi; ++it) {  // (hi - lo halves: 32 steps cover any int range)
        const int mid = lo + ((hi - lo) >> 1);
        const int t = c.child_tok[mid];
        if (t == k) return mid;
        if (t < k) lo = mid + 1; else hi = mid;
    }
    return -1;
}
// step(n, k) of the definition: m = n; while m is not the root and k is no child of m: m = fail(m); m' = child(m, k) or the root
__device__ __forceinline__ BeamStep beam_ctx_step(const BeamCtx &c, int n, int k)
{
    n = beam_ctx_node(c, n);
    int m = n, ch = -1;
    for (int hop = 0; hop <= BEAM_CTX_DEPTH; ++hop) {
        ch = beam_ctx_child(c, m, k);
        if (ch >= 0 || m == 0) break;
        m = beam_ctx_node(c, c.fail[m]);
    }
    const int mp = ch >= 0 ? beam_ctx_node(c, c.child_node[ch]) : 0;
    BeamStep s;
    s.next = c.terminal[mp] ? 0 : mp;
    s.ddepth = beam_ctx_depth(c, mp) - beam_ctx_depth(c, n);
    return s;
}
__device__ __forceinline__ double beam_ctx_delta(const BeamCtx &c, int ddepth) { return c.score * (double)ddepth; }

// the batched search's arguments (the kernels' trailing pack)
struct BeamBatch {
    size_t stride;        // bytes from one utterance's block of the workspace to the next
    const int32_t *utt;   // [N][2]: the utterance's first row of the packed frames, its frame count
    int rows;             // rows of the packed frames (row indices are kept below it)
    unsigned *n_done;     // zeroed device word: searches that have ended
};
__device__ __forceinline__ BeamBatch beam_batch() { return BeamBatch{0, nullptr, 0, nullptr}; }  // the single search
__device__ __forceinline__ BeamBatch beam_batch(const BeamBatch &b) { return b; }
// the streaming search's arguments: the batch's, over the caller's block
struct BeamStream {
    size_t stride;        // bytes from one stream's part of the block to the next
    const int32_t *push;  // [N][2]: the stream's first row of this push's packed frames, its frame count (0: the stream sits this push out)
    int rows;             // rows of the packed frames
    unsigned *n_rest;     // device word: streams at rest in this push
};
__device__ __forceinline__ BeamBatch beam_batch(const BeamStream &s) { return BeamBatch{s.stride, s.push, s.rows, s.n_rest}; }
// a search with a context graph: its BeamCtx ends the pack of k_beam_reduce and k_beam_select (the other kernels never see it)
__device__ __forceinline__ BeamBatch beam_batch(const BeamCtx &) { return beam_batch(); }
__device__ __forceinline__ BeamBatch beam_batch(const BeamBatch &b, const BeamCtx &) { return b; }
__device__ __forceinline__ const BeamCtx &beam_ctx(const BeamCtx &c) { return c; }
__device__ __forceinline__ const BeamCtx &beam_ctx(const BeamBatch &, const BeamCtx &c) { return c; }
// a search with the LSTMPredictor (DESIGN.md §4h "LSTM"): a BeamLstm ends the pack of k_beam_select only — the batched search whose selection
// also moves the hypotheses' LSTM state, as an INDEX: a hypothesis owns one of its utterance's 32 rows of the state pool
struct BeamLstm {
    int *srow;        // [2][BM] per utterance (double-buffered like len and hash): the pool row (0 .. 31) that holds the slot's state
    int *own, *par;   // [n_utt][BM] for the next round's predictor step: 32 u + the slot's row | 32 u + the row of the state it continues
};
__device__ __forceinline__ BeamBatch beam_batch(const BeamBatch &b, const BeamLstm &) { return b; }
__device__ __forceinline__ const BeamLstm &beam_lstm(const BeamBatch &, const BeamLstm &l) { return l; }
template <typename... U> struct beam_has_lstm { static constexpr bool value = false; };
template <> struct beam_has_lstm<BeamBatch, BeamLstm> { static constexpr bool value = true; };
template <typename... U> struct beam_has_ctx { static constexpr bool value = false; };
template <> struct beam_has_ctx<BeamCtx> { static constexpr bool value = true; };
template <> struct beam_has_ctx<BeamBatch, BeamCtx> { static constexpr bool value = true; };
template <typename... U> struct beam_batched { static constexpr bool value = sizeof...(U) > (beam_has_ctx<U...>::value ? 1 : 0); };
template <typename... U> struct beam_streams { static constexpr bool value = false; };
template <> struct beam_streams<BeamStream> { static constexpr bool value = true; };
// the word that stops a search's kernels: `done`, a stream's `at rest`
template <typename... U> __device__ __forceinline__ int beam_idle(const int32_t *state) { return state[beam_streams<U...>::value ? BS_REST : BS_DONE]; }
#define BEAM_UTT(ub) const BeamBatch B = beam_batch(ub...); const unsigned u = beam_batched<U...>::value ? blockIdx.y : 0u; const size_t uoff = u * B.stride

struct BeamSlots {
    double *score;               // [2][BM]
    unsigned long long *hash;    // [2][BM]  hash of the token sequence (pre-filter of the merges)
    int *len, *status, *need;    // [2][BM]  tokens after the leading blank | SL_* | text vector still to compute
    int *tok;                    // [2][BM][max_length]: tok[.][.][0] = blank, [1 .. len] the labels
    float *pvec;                 // [2][BM][H]: the joint's text input of the slot's sequence (after text_ln / LayerNorm)
};
__device__ __forceinline__ BeamSlots beam_utt(BeamSlots P, size_t stride)
{
    P.score = beam_utt(P.score, stride); P.hash = beam_utt(P.hash, stride); P.len = beam_utt(P.len, stride);
    P.status = beam_utt(P.status, stride); P.need = beam_utt(P.need, stride); P.tok = beam_utt(P.tok, stride);
    P.pvec = beam_utt(P.pvec, stride);
    return P;
}

__device__ __forceinline__ double beam_logaddexp(double a, double b)
{
    const double m = fmax(a, b);
    if (m == -__builtin_inf()) return m;
    return m + log1p(exp(-fabs(a - b)));
}

// ---- start of a search: slot 0 of buffer 0 = the empty hypothesis (score 0, text vector to compute), everything else empty
// (the workspace was zero-filled by the launcher: no value of a previous call, or of the caller's memory, is ever read)
template <typename... U> __global__ void k_beam_init(BeamSlots P, int32_t *state, int blank, int max_length, U... ub)
{
    if (threadIdx.x != 0) return;
    BEAM_UTT(ub);
    P = beam_utt(P, uoff); state += 32 * u;
    P.status[0] = SL_ACTIVE; P.need[0] = 1; P.len[0] = 0; P.score[0] = 0.0; P.hash[0] = 0ull;
    P.tok[0] = blank;
    for (int i = 0; i < 32; ++i) state[i] = 0;
    state[BS_N] = 1; state[BS_NEW] = 1;
}

// ---- conv1 outputs of positions p-4 .. p of every slot awaiting its predictor step (p = len: the newest token), as
// g1[slot][q][E], q = 0 .. 4 (zero rows before position 0 = conv2's left padding):
//   g1[pos] = gelu(b1 + A2[tok pos] + A1[tok pos-1] + A0[tok pos-2])      (rnnt/predictor.py:214-219, eval mode)
template <typename... U>
__global__ __launch_bounds__(256) void k_beam_conv1(const int32_t *__restrict__ state, BeamSlots P, int max_length, int S, int E,
                                                    const float *__restrict__ tab, const float *__restrict__ b1, float *__restrict__ g1, U... ub)
{
    BEAM_UTT(ub);
    state += 32 * u;
    if (beam_idle<U...>(state) || !state[BS_NEW]) return;
    P = beam_utt(P, uoff); g1 = beam_utt(g1, uoff);
    const int cur = state[BS_CUR], j = blockIdx.x;
    if (!P.need[cur * BM + j]) return;
    const int p = P.len[cur * BM + j];
    const int *tk = P.tok + ((size_t)cur * BM + j) * max_length;
    for (int q = 0; q < 5; ++q) {
        const int pos = p - 4 + q;
        float *out = g1 + ((size_t)j * 5 + q) * E;
        if (pos < 0) {
            for (int i = threadIdx.x; i < E; i += 256) out[i] = 0.f;
            continue;
        }
        auto row = [&](int at, int tap) {
            int s = tk[at];
            s = s < 0 ? 0 : (s >= S ? S - 1 : s);
            return tab + (size_t)s * 3 * E + (size_t)tap * E;
        };
        const float *a2 = row(pos, 2), *a1 = pos >= 1 ? row(pos - 1, 1) : nullptr, *a0 = pos >= 2 ? row(pos - 2, 0) : nullptr;
        for (int i = threadIdx.x; i < E; i += 256) {
            float v = b1[i] + a2[i];
            if (a1) v += a1[i];
            if (a0) v += a0[i];
            out[i] = gelu_erf(v);
        }
    }
}

// ---- Y[16][N] = act(bias + X[16][taps*Kin] . W^T) for the 16 slots.  W element (n, tap*Kin + i) at W[(tap*N + n)*Kin + i]:
// taps = 1 is torch.nn.Linear's [N][K], taps = 5 the [tap][out][in] conv pack.  LNIN: X is LN(z) * gamma + beta of the rows
// of `X` (Kin = taps * Kin features), normalised by the workgroup itself.  A workgroup: 16 outputs, its 4 waves split the
// reduction (16 k per chunk: a float4 per lane and operand -> 4 MFMAs, the k order inside the chunk permuted alike for both),
// partial tiles meet in LDS.  `masked`: only rows of slots awaiting their predictor step are written, into the CURRENT
// buffer (Y + cur * y_par).  Kin % 4 == 0, ldx % 4 == 0.  state, need, X and Y are the utterance's.
template <bool LNIN, typename... U>
__global__ __launch_bounds__(256) void k_beam_gemm16(const int32_t *__restrict__ state, const int *__restrict__ need,
                                                     const float *__restrict__ X, int ldx, const float *__restrict__ W, int taps, int Kin,
                                                     int N, const float *__restrict__ bias, int act, const float *__restrict__ gamma,
                                                     const float *__restrict__ beta, float eps, float *__restrict__ Y, int ldy,
                                                     long y_par, int masked, U... ub)
{
    __shared__ float s_acc[4][16][17];
    __shared__ float s_mean[16], s_rstd[16];
    BEAM_UTT(ub);
    state += 32 * u;
    if (beam_idle<U...>(state) || !state[BS_NEW]) return;
    need = beam_utt(need, uoff); X = beam_utt(X, uoff); Y = beam_utt(Y, uoff);
    const int cur = state[BS_CUR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16, ncol = min(n0 + r, N - 1);
    const int Kred = taps * Kin;
    if (LNIN) {  // mean / rstd of the 16 rows (two passes, a wave per 4 rows)
        for (int rr = wave * 4; rr < wave * 4 + 4; ++rr) {
            const float *x = X + (size_t)rr * ldx;
            float s = 0.f;
            for (int i = lane; i < Kred; i += 64) s += x[i];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
            const float mean = s / Kred;
            float s2 = 0.f;
            for (int i = lane; i < Kred; i += 64) { const float d = x[i] - mean; s2 += d * d; }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) s2 += __shfl_xor(s2, m, 64);
            if (lane == 0) { s_mean[rr] = mean; s_rstd[rr] = rsqrtf(s2 / Kred + eps); }
        }
        __syncthreads();
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const float *xr = X + (size_t)r * ldx;
    const int nchunk = (Kred + 15) / 16;
    for (int c = wave; c < nchunk; c += 4) {
        const int k = 16 * c + 4 * g;
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (k < Kred) {  // (Kred % 4 == 0: the whole float4 is in range)
            a = *(const f32x4 *)(xr + k);
            if (LNIN) {
                const f32x4 ga = *(const f32x4 *)(gamma + k), be = *(const f32x4 *)(beta + k);
                a = (a - s_mean[r]) * s_rstd[r] * ga + be;
            }
            const int tap = k / Kin, i = k - tap * Kin;
            b = *(const f32x4 *)(W + ((size_t)tap * N + ncol) * Kin + i);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s_acc[wave][4 * g + i][r] = acc[i];  // D: row (slot) 4 (lane >> 4) + i, column lane & 15
    __syncthreads();
    const int row = threadIdx.x >> 4, col = threadIdx.x & 15, n = n0 + col;
    if (n >= N || (masked && !need[cur * BM + row])) return;
    float v = ((s_acc[0][row][col] + s_acc[1][row][col]) + (s_acc[2][row][col] + s_acc[3][row][col])) + (bias ? bias[n] : 0.f);
    if (act) v = gelu_erf(v);
    Y[(masked ? (size_t)cur * y_par : 0) + (size_t)row * ldy + n] = v;
}

// ---- the predictor's output LayerNorm (rnnt/predictor.py:229) as the joint's text vector when the joint has no text_ln
template <typename... U>
__global__ __launch_bounds__(256) void k_beam_ln16(const int32_t *__restrict__ state, const int *__restrict__ need, const float *__restrict__ z,
                                                   int O, const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
                                                   float *__restrict__ pvec, U... ub)
{
    __shared__ float red[4];
    BEAM_UTT(ub);
    state += 32 * u;
    if (beam_idle<U...>(state) || !state[BS_NEW]) return;
    need = beam_utt(need, uoff); z = beam_utt(z, uoff); pvec = beam_utt(pvec, uoff);
    const int cur = state[BS_CUR], j = blockIdx.x;
    if (!need[cur * BM + j]) return;
    const float *x = z + (size_t)j * O;
    float mean, rstd;
    row_ln_stats(x, O, eps, red, mean, rstd);
    float *y = pvec + ((size_t)cur * BM + j) * O;
    for (int i = threadIdx.x; i < O; i += 256) y[i] = (x[i] - mean) * rstd * gamma[i] + beta[i];
}

// ---- logits[slot][v] = tanh(frame_t + pvec[slot]) . W[v] + bias[v] for all 16 slots, 16 vocabulary entries per workgroup
// (rnnt/joint.py:44-55 after the projections).  The hidden operand is built in registers: lane (slot r, k group g) takes
// tanh of its own sums, each element once per workgroup.  H % 4 == 0.  Batched search: frame t of the utterance is row
// utt[u][0] + t of the packed `frames`, kept inside the `rows` rows the caller vouched for; a stream's: row push[u][0] + (t - base).
template <typename... U>
__global__ __launch_bounds__(256) void k_beam_joint(const int32_t *__restrict__ state, const float *__restrict__ frames, long fstride,
                                                    const float *__restrict__ pvec, const float *__restrict__ W, const float *__restrict__ bias,
                                                    int H, int V, float *__restrict__ logits, U... ub)
{
    __shared__ float s_acc[4][16][17];
    BEAM_UTT(ub);
    state += 32 * u;
    if (beam_idle<U...>(state)) return;
    pvec = beam_utt(pvec, uoff); logits = beam_utt(logits, uoff);
    const int cur = state[BS_CUR];
    // (a stream: row = the push's first row + frames consumed since the push began)
    const int t = sizeof...(U) ? max(0, min(B.utt[2 * u] + state[BS_T] - (beam_streams<U...>::value ? state[BS_BASE] : 0), B.rows - 1)) : state[BS_T];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int v0 = blockIdx.x * 16, vcol = min(v0 + r, V - 1);
    const float *f = frames + (size_t)t * fstride, *pv = pvec + ((size_t)cur * BM + r) * H, *wr = W + (size_t)vcol * H;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int nchunk = (H + 15) / 16;
    for (int c = wave; c < nchunk; c += 4) {
        const int k = 16 * c + 4 * g;
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (k < H) {
            const f32x4 e = *(const f32x4 *)(f + k), p = *(const f32x4 *)(pv + k);
            b = *(const f32x4 *)(wr + k);
#pragma unroll
            for (int s = 0; s < 4; ++s) a[s] = fast_tanh(e[s] + p[s]);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) s_acc[wave][4 * g + i][r] = acc[i];
    __syncthreads();
    const int row = threadIdx.x >> 4, col = threadIdx.x & 15, v = v0 + col;
    if (v >= V) return;
    logits[(size_t)row * V + v] = ((s_acc[0][row][col] + s_acc[1][row][col]) + (s_acc[2][row][col] + s_acc[3][row][col])) + bias[v];
}

// (value, id) order of the label lists: larger value first, then the lower id
__device__ __forceinline__ bool beam_before(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

__device__ __forceinline__ void beam_wave_best(float &v, int &id)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(v, m, 64);
        const int oi = __shfl_xor(id, m, 64);
        if (beam_before(ov, oi, v, id)) { v = ov; id = oi; }
    }
}

// ---- per active slot (a workgroup of 16 waves each): log-sum-exp of the V logits, the blank logit and the `beam` best
// non-blank labels.  Waves walk 256-entry chunks, merging each into a running list of `beam` entries (lane q holds entry q)
// by `beam` wave-wide extractions; wave 0 merges the 16 lists the same way.
// CTX (the pack ends with a BeamCtx): the labels are ranked by their BIASED value logit + delta(n, k) at the slot's node n.  Every label that
// lands on the root shares the constant -bonus(n) and no label has a smaller delta, so of those the raw top-`beam` suffice; the others are
// the EXCEPTIONS: the children of the nodes of the fail chain n, fail(n), .., root (step() takes a label at the nearest node that has it).
// Wave 0 merges the raw list and the exceptions, 64 at a time, into the list it writes — with each label's RAW logit: k_beam_select
// recomputes step() and adds the delta in fp64.  No step() here: a chain walk and one level of loads per node.
template <typename... U>
__global__ __launch_bounds__(1024) void k_beam_reduce(const int32_t *__restrict__ state, const int *__restrict__ status,
                                                      const float *__restrict__ logits, int V, int blank, int beam, float *__restrict__ red,
                                                      U... ub)
{
    constexpr bool CTX = beam_has_ctx<U...>::value;
    __shared__ float s_v[16][BM], s_m[16], s_s[16];
    __shared__ int s_i[16][BM];
    BEAM_UTT(ub);
    state += 32 * u;
    if (beam_idle<U...>(state)) return;
    status = beam_utt(status, uoff); logits = beam_utt(logits, uoff); red = beam_utt(red, uoff);
    const int cur = state[BS_CUR], j = blockIdx.x;
    if (status[cur * BM + j] != SL_ACTIVE) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *x = logits + (size_t)j * V;
    const float NEG = RNNT_NEG_INF;
    const int NONE = 0x7fffffff;
    float lm = NEG, ls = 0.f;            // this lane's running (max, sum of exp)
    float lv = NEG;                      // entry `lane` of the wave's list
    int li = NONE;
    for (int c0 = wave * 256; c0 < V; c0 += 16 * 256) {
        const int v = c0 + 4 * lane;
        float cv[5];
        int ci[5];
        if (v < V) {  // V % 4 == 0
            const f32x4 q = *(const f32x4 *)(x + v);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y = q[e];
                if (y > lm) { ls = ls * expf(lm - y) + 1.f; lm = y; }
                else ls += expf(y - lm);
                cv[e] = (v + e == blank) ? NEG : y;
                ci[e] = (v + e == blank) ? NONE : v + e;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { cv[e] = NEG; ci[e] = NONE; }
        }
        cv[4] = lv; ci[4] = li;
        float nv = NEG;
        int ni = NONE;
        for (int q = 0; q < beam; ++q) {
            float bv = cv[0];
            int bi = ci[0], bw = 0;
#pragma unroll
            for (int e = 1; e < 5; ++e)
                if (beam_before(cv[e], ci[e], bv, bi)) { bv = cv[e]; bi = ci[e]; bw = e; }
            float wv = bv;
            int wi = bi;
            beam_wave_best(wv, wi);
            if (lane == q) { nv = wv; ni = wi; }
            if (wi != NONE && bi == wi) {  // the owner drops the extracted entry (ids are unique)
#pragma unroll
                for (int e = 0; e < 5; ++e)
                    if (e == bw) { cv[e] = NEG; ci[e] = NONE; }
            }
        }
        lv = nv; li = ni;
    }
    // the wave's (max, sum): combine the lanes
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float om = __shfl_xor(lm, m, 64), os = __shfl_xor(ls, m, 64);
        const float nm = fmaxf(lm, om);
        if (nm != NEG) {
            ls = (lm == NEG ? 0.f : ls * expf(lm - nm)) + (om == NEG ? 0.f : os * expf(om - nm));
            lm = nm;
        }
    }
    if (lane == 0) { s_m[wave] = lm; s_s[wave] = ls; }
    if (lane < BM) { s_v[wave][lane] = lane < beam ? lv : NEG; s_i[wave][lane] = lane < beam ? li : NONE; }
    __syncthreads();
    if (wave != 0) return;
    float cv[4];
    int ci[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = 4 * lane + e;  // 256 entries: list k >> 4, entry k & 15
        cv[e] = s_v[k >> 4][k & 15];
        ci[e] = s_i[k >> 4][k & 15];
    }
    float *out = red + (size_t)j * BEAM_RED;
    float fv = NEG;  // (CTX) entry `lane` of the raw list
    int fi = NONE;
    for (int q = 0; q < beam; ++q) {
        float bv = cv[0];
        int bi = ci[0], bw = 0;
#pragma unroll
        for (int e = 1; e < 4; ++e)
            if (beam_before(cv[e], ci[e], bv, bi)) { bv = cv[e]; bi = ci[e]; bw = e; }
        float wv = bv;
        int wi = bi;
        beam_wave_best(wv, wi);
        if constexpr (CTX) { if (lane == q) { fv = wv; fi = wi; } }
        else if (lane == 0) { out[16 + 2 * q] = wv; out[17 + 2 * q] = __int_as_float(wi); }
        if (wi != NONE && bi == wi) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e == bw) { cv[e] = NEG; ci[e] = NONE; }
        }
    }
    if (lane == 0) {
        float M = NEG;
        for (int w = 0; w < 16; ++w) M = fmaxf(M, s_m[w]);
        float S = 0.f;
        for (int w = 0; w < 16; ++w)
            if (s_m[w] != NEG) S += s_s[w] * expf(s_m[w] - M);
        out[0] = M + logf(S);
        out[1] = x[blank];
    }
    if constexpr (CTX) {
        const BeamCtx &cx = beam_ctx(ub...);
        const int n = beam_ctx_node(cx, beam_utt(cx.node, uoff)[cur * BM + j]);
        float rv = NEG;  // entry `lane` of the biased list
        int ri = NONE;
        auto merge = [&](float nv, int ni) {  // the best `beam` of the list and one new candidate per lane (every copy of an extracted id goes)
            float mv[2] = {nv, rv};
            int mi[2] = {ni, ri};
            float ov = NEG;
            int oi = NONE;
            for (int q = 0; q < beam; ++q) {
                const bool first = beam_before(mv[0], mi[0], mv[1], mi[1]);
                float wv = first ? mv[0] : mv[1];
                int wi = first ? mi[0] : mi[1];
                beam_wave_best(wv, wi);
                if (lane == q) { ov = wv; oi = wi; }
                if (wi != NONE) {
#pragma unroll
                    for (int e = 0; e < 2; ++e)
                        if (mi[e] == wi) { mv[e] = NEG; mi[e] = NONE; }
                }
            }
            rv = ov; ri = oi;
        };
        // Copies of one label are told apart by value alone: the copy of the NEAREST chain node is the deepest match, so the largest, and a
        // raw entry is entered as if it landed on the root — the smallest delta there is (delta >= -bonus(n)) —, so of a label's copies the
        // true one is extracted first and takes the others with it.  A stale copy can only keep out what the true copy would keep out.
        const int dn = beam_ctx_depth(cx, n);
        merge(lane < beam && fi != NONE ? fv + (float)beam_ctx_delta(cx, -dn) : NEG, lane < beam ? fi : NONE);
        int m = n;
        for (int hop = 0; hop <= BEAM_CTX_DEPTH; ++hop) {  // (m, lo, hi are the same in every lane)
            int lo, hi;
            beam_ctx_range(cx, m, lo, hi);
            const int up = m ? beam_ctx_node(cx, cx.fail[m]) : 0;
            for (int c0 = lo; c0 < hi; c0 += 64) {
                float nv = NEG;
                int ni = NONE;
                const int c = c0 + lane;
                if (c < hi) {
                    const int k = cx.child_tok[c];
                    if (k >= 0 && k < V && k != blank) {
                        nv = x[k] + (float)beam_ctx_delta(cx, beam_ctx_depth(cx, beam_ctx_node(cx, cx.child_node[c])) - dn);
                        ni = k;
                    }
                }
                merge(nv, ni);
            }
            if (m == 0) break;
            m = up;
        }
        if (lane < beam) {
            out[16 + 2 * lane] = ri != NONE ? x[ri] : NEG;
            out[17 + 2 * lane] = __int_as_float(ri);
        }
    }
}

__device__ bool beam_same_prefix(const int *a, const int *b, int len)  // positions 1 .. len
{
    for (int i = 1; i <= len; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

// ---- one workgroup per utterance: the selection of the round and the search's bookkeeping.  Batched search
// (T then unused: the utterance's frame count is utt[u][1]): the search that ends counts itself in `n_done` and the one that
// brings it to the n_utt = gridDim.y searches raises the host's flag.  A stream (T = base + push[u][1]) comes to REST there instead: the
// same result, the same count (k_beam_stream_begin counted the streams without frames), and the next push resumes from this very state.
// CTX (the pack ends with a BeamCtx): a label candidate's score takes delta(n, k) of its parent's node n in fp64 and its node is step(n, k)'s;
// finished, blank and merged candidates keep their source's node (a node is a function of the token sequence).  The scores it keeps
// and returns are INTERNAL: the bonus of an unfinished match is still in them (include/rnnt_engine.h: the finalisation rule).
template <typename... U>
__global__ __launch_bounds__(256) void k_beam_select(BeamSlots P, const float *__restrict__ red, int beam, int V, int H, int T, int max_length,
                                                     int max_per_frame, int32_t *__restrict__ state, int32_t *__restrict__ out_tokens,
                                                     double *__restrict__ out_scores, int32_t *host_flag, U... ub)
{
    constexpr bool CTX = beam_has_ctx<U...>::value, LSTM = beam_has_lstm<U...>::value;
    __shared__ int c_node[CTX ? BEAM_NC : 1], o_node[CTX ? BM : 1], o_row[LSTM ? BM : 1];
    __shared__ double c_score[BEAM_NC];
    __shared__ int c_kind[BEAM_NC], c_a[BEAM_NC], c_b[BEAM_NC], c_src[BEAM_NC];
    __shared__ unsigned char c_valid[BEAM_NC];
    __shared__ double o_score[BM];
    __shared__ unsigned long long o_hash[BM];
    __shared__ int o_len[BM], o_st[BM], s_bmatch[BM], s_keep[BM], s_final[BM];
    __shared__ int s_nfinal, s_frame_end, s_done;
    BEAM_UTT(ub);
    state += 32 * u;
    if (beam_idle<U...>(state)) return;
    P = beam_utt(P, uoff); red = beam_utt(red, uoff);
    out_tokens += (size_t)u * beam * max_length; out_scores += (size_t)u * beam;
    if (beam_batched<U...>::value) T = B.utt[2 * u + 1] + (beam_streams<U...>::value ? state[BS_BASE] : 0);  // a stream: the frame its push ends before
    const int tid = threadIdx.x, cur = state[BS_CUR], nb = cur ^ 1, r = state[BS_R];
    const int *tok_old = P.tok + (size_t)cur * BM * max_length;
    if (tid < BM) {
        const int idx = cur * BM + tid;
        o_st[tid] = tid < beam ? P.status[idx] : SL_EMPTY;
        o_score[tid] = P.score[idx]; o_hash[tid] = P.hash[idx]; o_len[tid] = P.len[idx];
        if constexpr (CTX) o_node[tid] = beam_ctx_node(beam_ctx(ub...), beam_utt(beam_ctx(ub...).node, uoff)[idx]);
        if constexpr (LSTM) o_row[tid] = beam_utt(beam_lstm(ub...).srow, uoff)[idx] & 31;
    }
    if (tid < BM) s_keep[tid] = -1;
    for (int c = tid; c < BEAM_NC; c += 256) c_valid[c] = 0;
    __syncthreads();
    // the finished entry each active slot's blank candidate merges with (the actives are distinct sequences, so are N's)
    if (tid < beam && o_st[tid] == SL_ACTIVE) {
        int mt = -1;
        for (int i = 0; i < beam && mt < 0; ++i)
            if (o_st[i] == SL_FINISHED && o_hash[i] == o_hash[tid] && o_len[i] == o_len[tid] &&
                beam_same_prefix(tok_old + (size_t)i * max_length, tok_old + (size_t)tid * max_length, o_len[tid]))
                mt = i;
        s_bmatch[tid] = mt;
    }
    // label candidates (parent j, its q-th label): at 32 + j * beam + q
    for (int c = tid; c < beam * beam; c += 256) {
        const int j = c / beam, q = c - j * beam, pos = 32 + c;
        if (o_st[j] != SL_ACTIVE || o_len[j] >= max_length - 1) continue;
        const float *rj = red + (size_t)j * BEAM_RED;
        const int id = __float_as_int(rj[17 + 2 * q]);
        if (id < 0 || id >= V) continue;
        c_score[pos] = o_score[j] + ((double)rj[16 + 2 * q] - (double)rj[0]);
        if constexpr (CTX) {
            const BeamStep s = beam_ctx_step(beam_ctx(ub...), o_node[j], id);
            c_score[pos] += beam_ctx_delta(beam_ctx(ub...), s.ddepth);
            c_node[pos] = s.next;
        }
        c_kind[pos] = 1; c_a[pos] = j; c_b[pos] = id; c_src[pos] = j; c_valid[pos] = 1;
    }
    __syncthreads();
    if (tid == 0) {  // N: the finished entries in slot order, then the unmerged blank candidates in slot order
        int nF = 0, fpos[BM];
        for (int i = 0; i < beam; ++i) {
            fpos[i] = -1;
            if (o_st[i] != SL_FINISHED) continue;
            c_score[nF] = o_score[i]; c_src[nF] = i; fpos[i] = nF++;
        }
        for (int j = 0; j < beam; ++j) {
            if (o_st[j] != SL_ACTIVE) continue;
            const float *rj = red + (size_t)j * BEAM_RED;
            const double bs = o_score[j] + ((double)rj[1] - (double)rj[0]);
            if (s_bmatch[j] >= 0) { const int k = fpos[s_bmatch[j]]; c_score[k] = beam_logaddexp(c_score[k], bs); }
            else { c_score[nF] = bs; c_src[nF] = j; ++nF; }
        }
        for (int f = 0; f < nF; ++f) { c_kind[f] = 0; c_a[f] = f; c_b[f] = 0; c_valid[f] = 1; }
    }
    __syncthreads();
    // rank of every candidate = how many beat it; the best `beam` are kept, at their rank
    const int ncand = 32 + beam * beam;
    for (int c = tid; c < ncand; c += 256) {
        if (!c_valid[c]) continue;
        const double sc = c_score[c];
        int rank = 0;
        for (int d = 0; d < ncand; ++d) {
            if (!c_valid[d] || d == c) continue;
            const double sd = c_score[d];
            const bool better = sd > sc || (sd == sc && (c_kind[d] < c_kind[c] || (c_kind[d] == c_kind[c] &&
                                                       (c_a[d] < c_a[c] || (c_a[d] == c_a[c] && c_b[d] < c_b[c])))));
            rank += better;
        }
        if (rank < beam) s_keep[rank] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int nk = 0;  // (the ranks are a permutation: keys are distinct)
        while (nk < beam && s_keep[nk] >= 0) ++nk;
        int nact = 0;
        for (int i = 0; i < nk; ++i) nact += c_kind[s_keep[i]];
        const int frame_end = nact == 0 || r >= max_per_frame - 1;
        int n = 0;
        if (frame_end && nact > 0) {  // the cap: kept labels join N without a blank term, merged by sequence
            for (int i = 0; i < nk; ++i)
                if (c_kind[s_keep[i]] == 0) s_final[n++] = s_keep[i];
            const int nfin = n;
            for (int i = 0; i < nk; ++i) {
                const int c = s_keep[i];
                if (c_kind[c] == 0) continue;
                const int src = c_src[c], len = o_len[src] + 1;
                const unsigned long long h = o_hash[src] * BEAM_HASH_MUL + (unsigned long long)(c_b[c] + 1);
                int hit = -1;
                for (int f = 0; f < nfin && hit < 0; ++f) {
                    const int fs = c_src[s_final[f]];
                    if (o_len[fs] != len || o_hash[fs] != h) continue;
                    const int *a = tok_old + (size_t)fs * max_length, *b = tok_old + (size_t)src * max_length;
                    if (a[len] == c_b[c] && beam_same_prefix(a, b, len - 1)) hit = f;
                }
                if (hit >= 0) c_score[s_final[hit]] = beam_logaddexp(c_score[s_final[hit]], c_score[c]);
                else s_final[n++] = c;
            }
            for (int i = 1; i < n; ++i) {  // stable: by score, finished before capped at equal scores
                const int c = s_final[i];
                int k = i;
                while (k > 0 && c_score[s_final[k - 1]] < c_score[c]) { s_final[k] = s_final[k - 1]; --k; }
                s_final[k] = c;
            }
        } else {
            for (int i = 0; i < nk; ++i) s_final[n++] = s_keep[i];
        }
        s_nfinal = n;
        s_frame_end = frame_end;
        s_done = frame_end && state[BS_T] + 1 >= T;
    }
    __syncthreads();
    const int n = s_nfinal, frame_end = s_frame_end, done = s_done;
    // the next slot buffer
    if (tid < BM) {
        const int idx = nb * BM + tid;
        if (tid < n) {
            const int c = s_final[tid], src = c_src[c], lab = c_kind[c];
            P.score[idx] = c_score[c];
            P.len[idx] = o_len[src] + lab;
            P.hash[idx] = lab ? o_hash[src] * BEAM_HASH_MUL + (unsigned long long)(c_b[c] + 1) : o_hash[src];
            P.status[idx] = frame_end || lab ? SL_ACTIVE : SL_FINISHED;
            P.need[idx] = lab;
            if constexpr (CTX) beam_utt(beam_ctx(ub...).node, uoff)[idx] = lab ? c_node[c] : o_node[src];
            if (done) { out_scores[tid] = c_score[c]; state[BS_LEN + tid] = o_len[src] + lab; }
        } else {
            P.score[idx] = -__builtin_inf(); P.len[idx] = 0; P.hash[idx] = 0ull; P.status[idx] = SL_EMPTY; P.need[idx] = 0;
            if constexpr (CTX) beam_utt(beam_ctx(ub...).node, uoff)[idx] = 0;
        }
        if constexpr (LSTM) {
            // A survivor (a capped label merged into a finished entry is one) keeps its row: nothing is copied.  The q-th kept label takes the
            // q-th row no slot of the current buffer refers to — at most 16 of the 32 are referred to, at most 16 labels are kept — and records
            // its parent's: siblings read one row and write different ones, and no row read in the next round's step is written in it.
            const BeamLstm &ls = beam_lstm(ub...);
            int mine = 0, parent = 0;
            if (tid < n) {
                const int c = s_final[tid];
                mine = parent = o_row[c_src[c]];
                if (c_kind[c]) {
                    unsigned used = 0u;
                    for (int i = 0; i < beam; ++i)
                        if (o_st[i] != SL_EMPTY) used |= 1u << o_row[i];
                    int q = 0;
                    for (int s = 0; s < tid; ++s) q += c_kind[s_final[s]];
                    unsigned freer = ~used;
                    for (int i = 0; i < q; ++i) freer &= freer - 1u;
                    mine = freer ? __builtin_ctz(freer) : 0;  // (never 0 by the count above)
                }
            }
            beam_utt(ls.srow, uoff)[idx] = mine;
            ls.own[u * BM + tid] = 32 * (int)u + mine;
            ls.par[u * BM + tid] = 32 * (int)u + parent;
        }
    }
    int *tok_new = P.tok + (size_t)nb * BM * max_length;
    for (int e = tid; e < n * max_length; e += 256) {
        const int s = e / max_length, i = e - s * max_length, c = s_final[s], src = c_src[c], len = o_len[src];
        int v;
        if (i <= len) v = tok_old[(size_t)src * max_length + i];
        else if (i == len + 1 && c_kind[c]) v = c_b[c];
        else continue;
        tok_new[(size_t)s * max_length + i] = v;
        if (done) out_tokens[(size_t)s * max_length + i] = v;
    }
    // text vectors move with their hypotheses (a new label's is computed by the next round's predictor step)
    const int H4 = H / 4;
    for (int e = tid; e < n * H4; e += 256) {
        const int s = e / H4, h = 4 * (e - s * H4), c = s_final[s];
        if (c_kind[c]) continue;
        *(f32x4 *)(P.pvec + ((size_t)nb * BM + s) * H + h) = *(const f32x4 *)(P.pvec + ((size_t)cur * BM + c_src[c]) * H + h);
    }
    if (tid == 0) {
        int any_new = 0;
        for (int s = 0; s < n; ++s) any_new |= c_kind[s_final[s]];
        state[BS_T] = state[BS_T] + frame_end;
        state[BS_R] = frame_end ? 0 : r + 1;
        state[BS_N] = n;
        state[BS_NEW] = any_new;
        state[BS_ROUNDS] += 1;
        state[BS_CUR] = nb;
        state[beam_streams<U...>::value ? BS_REST : BS_DONE] = done;  // a stream comes to rest: its result stands as at `done`, its search goes on
        // the host's cue to stop enqueueing rounds (mapped pinned memory, polled without a synchronisation)
        const bool all_done = done && (!beam_batched<U...>::value || atomicAdd(B.n_done, 1u) + 1 == gridDim.y);
        if (all_done && host_flag) __hip_atomic_store(host_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// ---- a stream's start: k_beam_init's state for stream `first + blockIdx.x` of the (zero-filled) block, at rest, and the
// result of zero frames: one entry, no labels, log-probability 0
__global__ void k_beam_stream_init(BeamSlots P, int32_t *state, double *scores, int blank, int beam, size_t stride, int first)
{
    if (threadIdx.x != 0) return;
    const unsigned u = first + blockIdx.x;
    P = beam_utt(P, u * stride); state += 32 * u;
    P.status[0] = SL_ACTIVE; P.need[0] = 1; P.len[0] = 0; P.score[0] = 0.0; P.hash[0] = 0ull;
    P.tok[0] = blank;
    for (int i = 0; i < 32; ++i) state[i] = 0;
    state[BS_N] = 1; state[BS_NEW] = 1; state[BS_REST] = 1;
    scores[(size_t)u * beam] = 0.0;
}

// ---- a push opens (one workgroup, a thread per stream): the frames consumed so far are the base of the push's rows; a stream that got
// frames leaves its rest, one that got none is counted as resting already.  All without frames: the flag rises here.
__global__ __launch_bounds__(64) void k_beam_stream_begin(int32_t *__restrict__ state, const int32_t *__restrict__ push, int n,
                                                          unsigned *__restrict__ n_rest, int32_t *host_flag)
{
    __shared__ unsigned s_idle;
    if (threadIdx.x == 0) s_idle = 0u;
    __syncthreads();
    if ((int)threadIdx.x < n) {
        int32_t *st = state + 32 * threadIdx.x;
        const int got = push[2 * threadIdx.x + 1] > 0;
        st[BS_BASE] = st[BS_T];
        st[BS_REST] = !got;
        if (!got) atomicAdd(&s_idle, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *n_rest = s_idle;
        if (s_idle == (unsigned)n && host_flag) __hip_atomic_store(host_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- workspace: per utterance { slot buffers | predictor intermediates | logits | reduce output }, `block` bytes each; then the
// batched search's done counter and the model's tables (when built here)
struct BeamLayout { size_t score, hash, len, status, need, tok, pvec, g1, g2, z, logits, red, node, block, n_done, state_end, tables, total; };
static BeamLayout beam_layout(int S, int E, int O, int H, int V, int has_text, int max_length, int n_utt, bool batched, bool ctx = false)
{
    BeamLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
    L.score = take(2 * BM * sizeof(double));
    L.hash = take(2 * BM * sizeof(unsigned long long));
    L.len = take(2 * BM * 4);
    L.status = take(2 * BM * 4);
    L.need = take(2 * BM * 4);
    L.tok = take((size_t)2 * BM * max_length * 4);
    L.pvec = take((size_t)2 * BM * H * 4);
    L.g1 = take((size_t)BM * 5 * E * 4);
    L.g2 = take((size_t)BM * E * 4);
    L.z = take((size_t)BM * O * 4);
    L.logits = take((size_t)BM * V * 4);
    L.red = take((size_t)BM * BEAM_RED * 4);
    L.node = take(ctx ? 2 * BM * 4 : 0);  // (a search with a context graph only: the others' layout is what it was)
    L.block = o;
    o *= (size_t)n_utt;
    L.n_done = take(batched ? 4 : 0);
    L.state_end = o;
    L.tables = take(dec_tables_floats(S, E, O, H, has_text) * 4);
    L.total = o;
    return L;
}
size_t beam_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, bool ctx)
{
    return beam_layout(S, E, O, H, V, has_text, max_length, 1, false, ctx).total;
}
size_t beam_batch_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int n_utt, bool ctx)
{
    return beam_layout(S, E, O, H, V, has_text, max_length, n_utt, true, ctx).total;
}
// a group of streams' persistent block: the batch's per-search parts and its counter (the tables are the caller's)
size_t beam_stream_block_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int n_streams)
{
    return beam_layout(S, E, O, H, V, has_text, max_length, n_streams, true).state_end;
}

template <typename Layout> static BeamSlots beam_slots(char *ws, const Layout &L)  // (BeamLayout, or the LSTM search's BeamLstmLayout)
{
    BeamSlots P;
    P.score = (double *)(ws + L.score); P.hash = (unsigned long long *)(ws + L.hash);
    P.len = (int *)(ws + L.len); P.status = (int *)(ws + L.status); P.need = (int *)(ws + L.need);
    P.tok = (int *)(ws + L.tok); P.pvec = (float *)(ws + L.pvec);
    return P;
}

// streams [first, first + count) of the block start over (count == n_streams: the whole block, its counter included)
void launch_beam_stream_init(void *block, int32_t *state, double *scores, int S, int E, int O, int H, int V, int has_text, int max_length,
                             int beam, int blank, int n_streams, int first, int count, hipStream_t st)
{
    const BeamLayout L = beam_layout(S, E, O, H, V, has_text, max_length, n_streams, true);
    char *ws = (char *)block;
    launch_fill32(ws + (size_t)first * L.block, 0u, count == n_streams ? L.state_end : (size_t)count * L.block, st);
    hipLaunchKernelGGL(k_beam_stream_init, dim3(count), dim3(64), 0, st, beam_slots(ws, L), state, scores, blank, beam, L.block, first);
}

// the single search (ba.utt == NULL: one utterance of a.T frames), the batched one (ba.n_utt utterances, rows of a.frames by ba.utt) and
// a push of ba.n_utt streams (ba.streaming: ba.utt is the push's table, a.workspace the streams' block, a.init = the push begins)
void launch_beam_decode(const BeamArgs &ba, hipStream_t st)
{
    const DecLoopArgs &a = ba.d;
    const int S = a.S, E = a.E, O = a.O, H = a.H, V = a.V, ML = a.max_length, has_text = a.text_W ? 1 : 0;
    const bool batched = ba.utt != nullptr;
    const unsigned N = batched ? ba.n_utt : 1;
    const bool ctx = ba.ctx != nullptr;  // (never with ba.streaming)
    const BeamLayout L = beam_layout(S, E, O, H, V, has_text, ML, N, batched, ctx);
    char *ws = (char *)a.workspace;
    const BeamSlots P = beam_slots(ws, L);
    BeamCtx cx{};
    if (ctx) {
        const rnnt_beam_context &g = *ba.ctx;
        cx = BeamCtx{g.child_off, g.child_tok, g.child_node, g.fail_link, g.depth, g.terminal, g.n_nodes, g.n_children, g.score, (int *)(ws + L.node)};
    }
    float *g1 = (float *)(ws + L.g1), *g2 = (float *)(ws + L.g2), *z = (float *)(ws + L.z);
    float *logits = (float *)(ws + L.logits), *red = (float *)(ws + L.red);
    const float *tb = (const float *)a.tables;
    if (a.init && !ba.streaming) launch_fill32(ws, 0u, L.state_end, st);
    if (!tb) {  // (rebuilt on every call that brings none: a function of the parameters only)
        launch_dec_build_tables(a.p, S, E, O, a.ln_in_eps, a.text_W, a.text_b, H, (float *)(ws + L.tables), st);
        tb = (const float *)(ws + L.tables);
    }
    size_t otab, owp2;
    dec_tables_offsets(S, E, O, H, has_text, &otab, &owp2);
    const float *tab = tb + otab, *wp2 = tb + owp2;
    const float *nul = nullptr;
    // `ub`: nothing (the single search's kernels) or the batch's BeamBatch; `with_ctx`: the reduce and the selection get the BeamCtx as the pack's last member
    // (a search with a context graph) — every other kernel, and every kernel of a search without one, is what it was
    auto enqueue_as = [&](auto with_ctx, auto... ub) {
        if (a.init && !ba.streaming)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_init<decltype(ub)...>), dim3(1, N), dim3(64), 0, st, P, a.state, a.blank, ML, ub...);
        for (int it = 0; it < a.iterations; ++it) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_conv1<decltype(ub)...>), dim3(BM, N), dim3(256), 0, st, a.state, P, ML, S, E, tab,
                               a.p.conv1_b, g1, ub...);
            // g2 = gelu(conv2(g1[p-4 .. p]))                                                  rnnt/predictor.py:222-223
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_gemm16<false, decltype(ub)...>), dim3((E + 15) / 16, N), dim3(256), 0, st, a.state, P.need,
                               g1, 5 * E, wp2, 5, E, E, a.p.conv2_b, 1, nul, nul, 0.f, g2, E, 0L, 0, ub...);
            // z = linear(g2)                                                                  rnnt/predictor.py:228
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_gemm16<false, decltype(ub)...>), dim3((O + 15) / 16, N), dim3(256), 0, st, a.state, P.need,
                               g2, E, a.p.linear_w, 1, E, O, a.p.linear_b, 0, nul, nul, 0.f, z, O, 0L, 0, ub...);
            // the slot's text vector: text_ln(LN(z)) (rnnt/joint.py:28-30) or LN(z) itself         rnnt/predictor.py:229
            if (has_text)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_gemm16<true, decltype(ub)...>), dim3((H + 15) / 16, N), dim3(256), 0, st, a.state,
                                   P.need, z, O, a.text_W, 1, O, H, a.text_b, 0, a.p.ln_out_w, a.p.ln_out_b, a.ln_eps, P.pvec, H, (long)BM * H, 1,
                                   ub...);
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_ln16<decltype(ub)...>), dim3(BM, N), dim3(256), 0, st, a.state, P.need, z, O,
                                   a.p.ln_out_w, a.p.ln_out_b, a.ln_eps, P.pvec, ub...);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_joint<decltype(ub)...>), dim3((V + 15) / 16, N), dim3(256), 0, st, a.state, a.frames,
                               a.frame_stride, P.pvec, a.W, a.bias, H, V, logits, ub...);
            if constexpr (decltype(with_ctx)::value) {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_reduce<decltype(ub)..., BeamCtx>), dim3(ba.beam, N), dim3(1024), 0, st, a.state,
                                   P.status, logits, V, a.blank, ba.beam, red, ub..., cx);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_select<decltype(ub)..., BeamCtx>), dim3(1, N), dim3(256), 0, st, P, red, ba.beam, V, H,
                                   a.T, ML, a.max_per_frame, a.state, a.tokens, ba.scores, a.host_flag, ub..., cx);
            } else {
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_reduce<decltype(ub)...>), dim3(ba.beam, N), dim3(1024), 0, st, a.state, P.status, logits,
                                   V, a.blank, ba.beam, red, ub...);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_select<decltype(ub)...>), dim3(1, N), dim3(256), 0, st, P, red, ba.beam, V, H, a.T, ML,
                                   a.max_per_frame, a.state, a.tokens, ba.scores, a.host_flag, ub...);
            }
        }
    };
    auto enqueue = [&](auto... ub) { enqueue_as(std::false_type{}, ub...); };
    auto enqueue_ctx = [&](auto... ub) { enqueue_as(std::true_type{}, ub...); };
    if (ba.streaming) {
        unsigned *n_rest = (unsigned *)(ws + L.n_done);
        if (a.init) hipLaunchKernelGGL(k_beam_stream_begin, dim3(1), dim3(64), 0, st, a.state, ba.utt, (int)N, n_rest, a.host_flag);
        enqueue(BeamStream{L.block, ba.utt, ba.rows, n_rest});
    } else if (ctx) {
        if (batched) enqueue_ctx(BeamBatch{L.block, ba.utt, ba.rows, (unsigned *)(ws + L.n_done)});
        else enqueue_ctx();
    } else if (batched)
        enqueue(BeamBatch{L.block, ba.utt, ba.rows, (unsigned *)(ws + L.n_done)});
    else
        enqueue();
}

// ---- the search with the LSTMPredictor (rnnt_engine_beam_decode_lstm; DESIGN.md §4h "LSTM"): the batched search, n_utt = 1 included, whose
// predictor step is lstm.hip's (launch_beam_lstm_step) and whose selection moves the LSTM state as an index into a pool of 32 rows per
// utterance.  Workspace: per utterance { slot buffers | logits | reduce output | state rows' indices }, then the done counter, the
// step's row indices, the pool — all zero-filled at init — and the step's scratch, of which no value outlives a round.
static_assert(BEAM_ST_DONE == BS_DONE && BEAM_ST_NEW == BS_NEW && BEAM_ST_CUR == BS_CUR, "the predictor step reads the search's state words");
struct BeamLstmLayout { size_t score, hash, len, status, need, tok, pvec, logits, red, srow, block, n_done, own, par, pool, state_end, scratch, total; };
static BeamLstmLayout beam_lstm_layout(int n_utt, int E, int Hd, int O, int L, int H, int V, int max_length)
{
    BeamLstmLayout w;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
    w.score = take(2 * BM * sizeof(double));
    w.hash = take(2 * BM * sizeof(unsigned long long));
    w.len = take(2 * BM * 4);
    w.status = take(2 * BM * 4);
    w.need = take(2 * BM * 4);
    w.tok = take((size_t)2 * BM * max_length * 4);
    w.pvec = take((size_t)2 * BM * H * 4);
    w.logits = take((size_t)BM * V * 4);
    w.red = take((size_t)BM * BEAM_RED * 4);
    w.srow = take(2 * BM * 4);
    w.block = o;
    o *= (size_t)n_utt;
    w.n_done = take(4);
    w.own = take((size_t)n_utt * BM * 4);
    w.par = take((size_t)n_utt * BM * 4);
    w.pool = take((size_t)n_utt * 32 * L * 2 * Hd * 4);
    w.state_end = o;
    w.scratch = take(beam_lstm_step_floats(n_utt, E, Hd, O, H) * 4);
    w.total = o;
    return w;
}
size_t beam_lstm_workspace_bytes(int n_utt, int E, int Hd, int O, int L, int H, int V, int max_length)
{
    return beam_lstm_layout(n_utt, E, Hd, O, L, H, V, max_length).total;
}

// the start: the empty hypothesis of every utterance continues the zero state of row 0 (the pool was zero-filled) and owns row 1
__global__ void k_beam_lstm_init(BeamLstm ls, size_t stride)
{
    const unsigned u = blockIdx.x, s = threadIdx.x;
    if (s >= BM) return;
    if (s == 0) beam_utt(ls.srow, u * stride)[0] = 1;
    ls.own[u * BM + s] = 32 * (int)u + (s == 0 ? 1 : 0);
    ls.par[u * BM + s] = 32 * (int)u;
}

void launch_beam_decode_lstm(const BeamLstmArgs &a, hipStream_t st)
{
    const BeamLstmStep &m = a.s;
    const int H = m.H, V = a.V, ML = m.max_length;
    const unsigned N = m.n_utt;
    const BeamLstmLayout w = beam_lstm_layout(N, m.E, m.Hd, m.O, m.L, H, V, ML);
    char *ws = (char *)a.workspace;
    const BeamSlots P = beam_slots(ws, w);
    float *logits = (float *)(ws + w.logits), *red = (float *)(ws + w.red);
    const BeamBatch bb{w.block, a.utt, a.rows, (unsigned *)(ws + w.n_done)};
    const BeamLstm ls{(int *)(ws + w.srow), (int *)(ws + w.own), (int *)(ws + w.par)};
    BeamLstmStep step = m;
    step.state = a.state; step.need = P.need; step.len = P.len; step.tok = P.tok; step.pvec = P.pvec; step.stride = w.block;
    step.own = ls.own; step.par = ls.par; step.pool = (float *)(ws + w.pool); step.scratch = (float *)(ws + w.scratch);
    if (a.init) {
        launch_fill32(ws, 0u, w.state_end, st);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_init<BeamBatch>), dim3(1, N), dim3(64), 0, st, P, a.state, a.blank, ML, bb);
        hipLaunchKernelGGL(k_beam_lstm_init, dim3(N), dim3(64), 0, st, ls, w.block);
    }
    for (int it = 0; it < a.iterations; ++it) {
        launch_beam_lstm_step(step, st);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_joint<BeamBatch>), dim3((V + 15) / 16, N), dim3(256), 0, st, a.state, a.frames, a.frame_stride,
                           P.pvec, a.W, a.bias, H, V, logits, bb);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_reduce<BeamBatch>), dim3(a.beam, N), dim3(1024), 0, st, a.state, P.status, logits, V, a.blank,
                           a.beam, red, bb);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_beam_select<BeamBatch, BeamLstm>), dim3(1, N), dim3(256), 0, st, P, red, a.beam, V, H, 0, ML,
                           a.max_per_frame, a.state, a.tokens, a.scores, a.host_flag, bb, ls);
    }
}
