// ctc.hip — CTC auxiliary head for gfx950: fused loss (forward + backward) and greedy decode.
//
//   k_ctc_gather   logits [N,T,V] -> per frame: the fp32 log-sum-exp denom[n,t], lp_blank[n,t], lp_label[n,t,u] (u < U_n)
//   k_ctc_links    per utterance: "next position with the same label" links, for the deterministic scatter of k_ctc_grad
//   k_ctc_chain    alpha / beta over the T x (2U+1) lattice, one workgroup per (utterance, direction), two states per lane
//                  (a failed chain — bounded spin ran out — turns every cost and log P of the call into NaN: launch_chain_status)
//   k_ctc_grad     d cost / d logits, one wave per frame, every sum in a fixed order
//   k_ctc_argmax, k_ctc_collapse   greedy decode: argmax per frame, then drop repeats and blanks per utterance
//
// State numbering: s = 2u is the blank before label u (u = 0 .. U_n; 2 U_n is the final blank), s = 2u + 1 is label u.
// alpha_t(s) and beta_t(s) both INCLUDE the emission of frame t, so the posterior occupancy of state s at frame t is
// exp(alpha + beta - lp_t(s) - log P).  alpha / beta are fp64 (they reach ~1e4 in magnitude and the occupancy needs
// alpha + beta - log P, a cancellation fp32 cannot hold to 1e-4); the log-add-exp correction is fp32 on exp2 / log2.
#include "lattice_common.hpp"  // wave_shift, lse2_safe, row_max_sumexp, chain_mailbox_bytes: shared with lattice.hip
#include "kernels.hpp"

#define CTC_NO_LINK 0xffff    // k_ctc_links: no later position carries this label
#define CTC_HEAD 0x10000      // k_ctc_links: no earlier position carries this label

// a label as every kernel reads it: held inside the vocabulary, so that a bad target indexes no logit outside its row
__device__ __forceinline__ int ctc_tok(const int32_t *__restrict__ targets, long i, int V)
{
    const int y = targets[i];
    return y < 0 ? 0 : (y >= V ? V - 1 : y);
}

// ---------------------------------------------------------------------------------------
// One wave per frame (n,t), V % 4 == 0.  Frames at t >= T_n are never read.
__global__ __launch_bounds__(256) void k_ctc_gather(
    const float *__restrict__ logits, const int32_t *__restrict__ targets, const int32_t *__restrict__ logit_lens,
    const int32_t *__restrict__ target_lens, float *__restrict__ denom, float *__restrict__ lpb, float *__restrict__ lpl,
    int N, int T, int U, int V, int blank)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)N * T) return;
    const int n = (int)(row / T), t = (int)(row - (long)n * T);
    if (t >= len_t(logit_lens, n, T)) return;
    const float *x = logits + row * V;
    float m, s;  // (a NaN logit is skipped by the max and lands in the sum: NaN denominator, NaN lp_blank, NaN cost)
    row_max_sumexp(x, V, lane, m, s);
    const float den = m + logf(s);
    if (lane == 0) {
        denom[row] = den;
        lpb[row] = x[blank] - den;
    }
    const int Un = len_u(target_lens, n, U + 1), Us = U > 0 ? U : 1;
    for (int u = lane; u < Un; u += 64) lpl[row * Us + u] = x[ctc_tok(targets, (long)n * U + u, V)] - den;
}

// ---------------------------------------------------------------------------------------
// link[n,u] = the next position u' > u with the same label (CTC_NO_LINK: none) | CTC_HEAD when no earlier position has it.
// One workgroup per utterance, the labels staged in LDS; U <= 1023.
__global__ __launch_bounds__(1024) void k_ctc_links(const int32_t *__restrict__ targets, const int32_t *__restrict__ target_lens,
                                                    int32_t *__restrict__ link, int U, int V)
{
    __shared__ int s_y[1024];
    const int n = blockIdx.x, u = threadIdx.x;
    const int Un = len_u(target_lens, n, U + 1);
    if (u < Un) s_y[u] = ctc_tok(targets, (long)n * U + u, V);
    __syncthreads();
    if (u >= Un) return;
    const int y = s_y[u];
    int nxt = CTC_NO_LINK, head = CTC_HEAD;
    for (int j = u + 1; j < Un; ++j)
        if (s_y[j] == y) { nxt = j; break; }
    for (int j = 0; j < u; ++j)
        if (s_y[j] == y) { head = 0; break; }
    link[(long)n * U + u] = nxt | head;
}

// ---------------------------------------------------------------------------------------
// log(exp a + exp b + exp c) with fp64 maximum and fp32 correction (< ln 3) on the hardware exp2 / log2; -inf-safe as lse2_safe is:
// a state INSIDE the lattice may have no reachable predecessor (and an infeasible utterance has none at the end)
__device__ __forceinline__ double ctc_lse3(double a, double b, double c)
{
    const double m = fmax(a, fmax(b, c));
    const bool dead = m == (double)RNNT_NEG_INF;
    const float da = dead ? 0.f : (float)(a - m), db = dead ? 0.f : (float)(b - m), dc = dead ? 0.f : (float)(c - m);
    const float s = __builtin_amdgcn_exp2f(da * RNNT_LOG2E) + __builtin_amdgcn_exp2f(db * RNNT_LOG2E) +
                    __builtin_amdgcn_exp2f(dc * RNNT_LOG2E);
    return m + (double)(__builtin_amdgcn_logf(s) * 0.6931471805599453f);
}

// One workgroup per (utterance, direction), stepping over the frames.  Lane j owns two states: the blank 2j and the label
// 2j + 1 of the sweep's OWN numbering — alpha's is the lattice's; beta runs the same recurrence on the reversed label
// sequence over reversed time (state s' = 2 U_n - s, frame T_n - 1 - k), so both directions are one body and move ONE value
// per step across lanes, the previous lane's label state:
//   blank'(j) = lp_blank + lse(blank(j), label(j-1))
//   label'(j) = lp_label + lse(label(j), blank(j), label(j-1) if the two labels differ)
// MBOX: the waves are not joined by a barrier per step; inside a wave the value moves by a DPP wave shift, at a wave
// boundary through an LDS mailbox [boundary][step] (value, then tag = step + 1; every slot written once, the consumer's spin
// bounded: lattice.hip's lattice_chain).  !MBOX (the mailboxes of NW - 1 boundaries x T steps do not fit in LDS): the
// boundary values cross through a double-buffered LDS line and one barrier per step.
// The beta half also writes log P (fp64, for k_ctc_grad) and costs[n] = -log P: +inf when no path exists, NaN when a
// frame t < T_n holds a NaN (its lp_blank is NaN; the sweep itself clamps every lp to <= 0, which drops NaNs).
template <int DIR, bool MBOX>
__device__ __forceinline__ void ctc_chain(
    const float *__restrict__ lpb_a, const float *__restrict__ lpl_a, double *__restrict__ out_a,
    const int32_t *__restrict__ targets, const int32_t *__restrict__ logit_lens, const int32_t *__restrict__ target_lens,
    float *__restrict__ costs, double *__restrict__ logp, int T, int U, int V, unsigned *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    __shared__ double s_fin[2];
    const int NW = blockDim.x >> 6;
    const int j = threadIdx.x, l = j & 63;
    const int w = __builtin_amdgcn_readfirstlane(j >> 6);
    typedef __attribute__((address_space(3))) volatile double lds_f64;
    typedef __attribute__((address_space(3))) volatile int lds_i32;
    lds_f64 *mval = (lds_f64 *)sm;                               // MBOX: [NW-1][T]; else the line [2][NW]
    lds_i32 *mtag = (lds_i32 *)(sm + (size_t)(NW - 1) * T);      // MBOX: [NW-1][T]
    const double NINF = (double)RNNT_NEG_INF;
    if (MBOX) {
        for (int i = j; i < (NW - 1) * T; i += blockDim.x) mtag[i] = 0;
    } else {
        for (int i = j; i < 2 * NW; i += blockDim.x) mval[i] = NINF;
    }
    if (j < 2) s_fin[j] = NINF;
    __syncthreads();

    const int n = blockIdx.x;
    const int Tn = len_t(logit_lens, n, T), Un = len_u(target_lens, n, U + 1);
    const int Us = U > 0 ? U : 1, S2 = 2 * (U + 1);
    const float *lpb = lpb_a + (long)n * T, *lpl = lpl_a + (long)n * T * Us;
    double *out = out_a + (long)n * T * S2;
    const bool b_ok = j <= Un, l_ok = j < Un;
    const int lab = DIR == 0 ? j : Un - 1 - j;                     // the label this lane's label state carries (l_ok)
    const int sb = DIR == 0 ? 2 * j : 2 * (Un - j), sl = DIR == 0 ? 2 * j + 1 : 2 * (Un - j) - 1;  // lattice state numbers
    const int labc = l_ok ? lab : 0;
    bool skip = false;  // the label state may be entered from the previous lane's label state
    if (l_ok && j > 0)
        skip = ctc_tok(targets, (long)n * U + lab, V) != ctc_tok(targets, (long)n * U + (DIR == 0 ? lab - 1 : lab + 1), V);

    bool bad = false;
    if (DIR == 1)
        for (int t = j; t < Tn; t += blockDim.x) { const float v = lpb[t]; bad = bad || v != v; }

    // a wave whose lanes all lie beyond U_n neither produces nor consumes (its neighbour below is the last one with states)
    const bool active = w * 64 <= Un;
    const bool has_prod = active && w < NW - 1 && (w + 1) * 64 <= Un, has_cons = active && w > 0;
    const int pbase = w * T, cbase = (w - 1) * T;

    auto frame = [&](int k) { const int kk = k < Tn ? k : Tn - 1; return DIR == 0 ? kk : Tn - 1 - kk; };
    auto fetch = [&](int k, float &lb, float &ll) {
        const int t = frame(k);
        lb = lpb[t];
        ll = lpl[(long)t * Us + labc];
    };
    auto store = [&](int k, double a0, double a1) {
        const long r = (long)frame(k) * S2;
        if (b_ok) out[r + sb] = a0;
        if (l_ok) out[r + sl] = a1;
    };

    double a0 = NINF, a1 = NINF;
    float lb, ll;
    fetch(0, lb, ll);
    if (MBOX ? active : true) {
        // ---- step 0: the first frame starts in the first blank or the first label
        float nlb, nll;
        fetch(1, nlb, nll);
        // fminf, not a bare v_min_f32: slots no kernel wrote may hold any bit pattern (lattice.hip, lattice_chain)
        a0 = j == 0 ? (double)fminf(lb, 0.f) : NINF;
        a1 = (j == 0 && l_ok) ? (double)fminf(ll, 0.f) : NINF;
        store(0, a0, a1);
        int tg = 0;
        double bv = NINF;
        bool gave_up = false;
        if (MBOX) {
            if (has_prod && l == 63) { mval[pbase] = a1; mtag[pbase] = 1; }
            if (has_cons) { tg = mtag[cbase]; bv = mval[cbase]; }
        } else {
            if (l == 63) mval[w] = a1;
            __syncthreads();
        }
        for (int k = 1; k < Tn; ++k) {
            lb = nlb; ll = nll;
            fetch(k + 1, nlb, nll);  // (clamped to the last frame inside)
            if (MBOX) {
                if (has_cons && !gave_up && tg != k) {  // wave-uniform; rare once the waves have settled a step apart
                    for (int spin = 0; tg != k && spin < (1 << 22); ++spin) { tg = mtag[cbase + k - 1]; bv = mval[cbase + k - 1]; }
                    // the producer never published step k - 1 (cannot happen while the workgroup is resident): raise the error
                    // word — k_chain_status then turns every cost of the call into NaN — and wait for nothing any more, so that
                    // a failed sweep still ends after ONE exhausted spin per wave
                    if (tg != k) {
                        gave_up = true;
                        if (l == 0) atomicOr(err, 1u);
                    }
                }
            } else {
                bv = w > 0 ? mval[((k - 1) & 1) * NW + w - 1] : NINF;
            }
            const double nb = wave_shift<0x138>(a1, bv);  // label state of lane j - 1 at step k - 1
            if (MBOX && has_cons) { tg = mtag[cbase + k]; bv = mval[cbase + k]; }  // next step's, early (k < T: the slot exists)
            const double v0 = (double)fminf(lb, 0.f) + lse2_safe(a0, nb);
            const double v1 = (double)fminf(ll, 0.f) + ctc_lse3(a1, a0, skip ? nb : NINF);
            a0 = b_ok ? v0 : NINF;
            a1 = l_ok ? v1 : NINF;
            if (MBOX) {
                if (has_prod && l == 63) { mval[pbase + k] = a1; mtag[pbase + k] = k + 1; }
            } else {
                if (l == 63) mval[(k & 1) * NW + w] = a1;
            }
            store(k, a0, a1);
            if (!MBOX) __syncthreads();  // (T_n is uniform over the workgroup: every wave passes the same barriers)
        }
    }
    // log P = lse(final blank, last label) after the last step: lanes U_n and U_n - 1 in either direction
    if (j == Un) s_fin[0] = a0;
    if (Un > 0 && j == Un - 1) s_fin[1] = a1;
    const int any_bad = __syncthreads_or(bad ? 1 : 0);  // (every wave arrives: all spins are bounded)
    if (DIR == 1 && j == 0) {
        const double lp = lse2_safe(s_fin[0], s_fin[1]);
        logp[n] = any_bad ? (double)__builtin_nanf("") : lp;
        costs[n] = any_bad ? __builtin_nanf("") : (float)(-lp);
    }
}

template <bool MBOX>
__global__ __launch_bounds__(1024) void k_ctc_chain(
    const float *__restrict__ lpb, const float *__restrict__ lpl, double *__restrict__ alpha, double *__restrict__ beta,
    const int32_t *__restrict__ targets, const int32_t *__restrict__ logit_lens, const int32_t *__restrict__ target_lens,
    float *__restrict__ costs, double *__restrict__ logp, int T, int U, int V, unsigned *__restrict__ err)
{
    if (blockIdx.y == 0)
        ctc_chain<0, MBOX>(lpb, lpl, alpha, targets, logit_lens, target_lens, costs, logp, T, U, V, err);
    else
        ctc_chain<1, MBOX>(lpb, lpl, beta, targets, logit_lens, target_lens, costs, logp, T, U, V, err);
}

// ---------------------------------------------------------------------------------------
// d (weight_n cost_n) / d logits[n,t,:] = weight_n (softmax - occupancy), one wave per frame.  Zero rows: t >= T_n, an
// infeasible utterance (log P = -inf), a zero weight.  The occupancies of the states that share a vocabulary entry are summed
// in a FIXED order — the blanks lane by lane and then by the butterfly, a label's positions along its chain of k_ctc_links by
// the lane that owns the first of them — and each entry of the row gets its final value by a plain store: no atomics, two
// runs give the same bits.  The row is written once as the softmax (blank included); after the wave's stores have landed,
// the owner of each label stores softmax - occupancy over its entry.
__device__ __forceinline__ float ctc_occupancy(const double *__restrict__ a, const double *__restrict__ b, long i, float lp_state,
                                               double lp)
{
    const double ab = a[i] + b[i];
    // (an unreachable state: nothing; also keeps (-inf) - (-inf) out when the state's own log-prob is -inf)
    return ab == (double)RNNT_NEG_INF ? 0.f : __expf((float)(ab - (double)fminf(lp_state, 0.f) - lp));
}

__global__ __launch_bounds__(256) void k_ctc_grad(
    const float *__restrict__ logits, const int32_t *__restrict__ targets, const int32_t *__restrict__ link,
    const int32_t *__restrict__ logit_lens, const int32_t *__restrict__ target_lens, const float *__restrict__ denom,
    const float *__restrict__ lpb, const float *__restrict__ lpl, const double *__restrict__ alpha,
    const double *__restrict__ beta, const double *__restrict__ logp, const float *__restrict__ weights,
    float *__restrict__ grad, int N, int T, int U, int V, int blank)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)N * T) return;
    const int n = (int)(row / T), t = (int)(row - (long)n * T);
    const float *x = logits + row * V;
    float *g = grad + row * V;
    const float wt = weights ? weights[n] : 1.0f;
    const double lp = logp[n];
    // (ordered compares: a NaN cost or weight keeps the row live and comes out as NaN)
    const bool live = t < len_t(logit_lens, n, T) && !(lp == (double)RNNT_NEG_INF) && !(wt == 0.f);
    if (!live) {
        for (int v = lane * 4; v < V; v += 256) *(f32x4 *)(g + v) = f32x4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const int Un = len_u(target_lens, n, U + 1), Us = U > 0 ? U : 1, S2 = 2 * (U + 1);
    const long st = row * S2;  // the states of this frame
    const float den = denom[row], lb = lpb[row];
    float occb = 0.f;
    for (int u = lane; u <= Un; u += 64) occb += ctc_occupancy(alpha, beta, st + 2 * u, lb, lp);
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) occb += __shfl_xor(occb, k, 64);
    for (int v = lane * 4; v < V; v += 256) {
        const f32x4 q = *(const f32x4 *)(x + v);
        f32x4 o;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            float e = __expf(q[s] - den);
            if (v + s == blank) e -= occb;
            o[s] = wt * e;
        }
        *(f32x4 *)(g + v) = o;
    }
    // the row's stores above are acknowledged before any lane stores over one of its entries
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int u = lane; u < Un; u += 64) {
        if (!(link[(long)n * U + u] & CTC_HEAD)) continue;
        float occ = 0.f;
        for (int p = u; p != CTC_NO_LINK; p = link[(long)n * U + p] & 0xffff)
            occ += ctc_occupancy(alpha, beta, st + 2 * p + 1, lpl[row * Us + p], lp);
        const int v = ctc_tok(targets, (long)n * U + u, V);
        float e = __expf(x[v] - den) - occ;
        if (v == blank) e -= occb;  // (a target that names the blank: outside the contract, still one defined value)
        g[v] = wt * e;
    }
}

// ---------------------------------------------------------------------------------------
// Greedy decode.  k_ctc_argmax: one wave per frame, tokens[n,t] = argmax (lowest index on ties; frames t >= T_n are not read).
// k_ctc_collapse: one workgroup per utterance compacts tokens[n,:] in place — a frame is kept when it is not the blank and
// differs from its predecessor — by a block scan over 1024 frames at a time; counts[n] = the kept frames.
__global__ __launch_bounds__(256) void k_ctc_argmax(const float *__restrict__ logits, const int32_t *__restrict__ logit_lens,
                                                    int32_t *__restrict__ tokens, int N, int T, int V)
{
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)N * T) return;
    const int n = (int)(row / T), t = (int)(row - (long)n * T);
    if (t >= len_t(logit_lens, n, T)) return;
    const float *x = logits + row * V;
    float best = RNNT_NEG_INF;
    int bi = 0x7fffffff;
    for (int v = lane * 4; v < V; v += 256) {  // V % 4 == 0
        const f32x4 q = *(const f32x4 *)(x + v);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (q[e] > best) { best = q[e]; bi = v + e; }  // increasing v: first index wins ties
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) tokens[row] = bi < V ? bi : 0;  // (a frame of NaN / -inf only: entry 0)
}

__global__ __launch_bounds__(1024) void k_ctc_collapse(const int32_t *__restrict__ logit_lens, int32_t *__restrict__ tokens,
                                                       int32_t *__restrict__ counts, int T, int blank)
{
    __shared__ int s_wave[16];
    __shared__ int s_base, s_last;
    const int n = blockIdx.x, j = threadIdx.x, lane = j & 63, wave = j >> 6;
    const int Tn = len_t(logit_lens, n, T);
    int32_t *tok = tokens + (long)n * T;
    if (j == 0) { s_base = 0; s_last = -1; }
    __syncthreads();
    for (int t0 = 0; t0 < Tn; t0 += 1024) {  // (uniform over the workgroup)
        const int t = t0 + j;
        const int cur = t < Tn ? tok[t] : blank;
        const int prev = j > 0 ? (t - 1 < Tn ? tok[t - 1] : blank) : s_last;  // the raw argmax, read before anything is stored
        const bool keep = t < Tn && cur != blank && cur != prev;
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wave] = __popcll(mask);
        const int base = s_base;
        __syncthreads();
        int off = base, total = base;
        for (int k = 0; k < 16; ++k) {
            if (k < wave) off += s_wave[k];
            total += s_wave[k];
        }
        if (keep) tok[off + before] = cur;  // off + before <= t: behind every frame still to be read
        __syncthreads();
        if (j == 1023) s_last = cur;
        if (j == 0) s_base = total;
        __syncthreads();
    }
    if (j == 0) counts[n] = s_base;
}

// ---------------------------------------------------------------------------------------
void launch_ctc_loss(const CtcArgs &a, hipStream_t st)
{
    const long rows = (long)a.N * a.T;
    const int NW = (a.U + 1 + 63) / 64;
    hipLaunchKernelGGL(k_ctc_gather, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a.logits, a.targets, a.logit_lens,
                       a.target_lens, a.denom, a.lpb, a.lpl, a.N, a.T, a.U, a.V, a.blank);
    const size_t mbox = chain_mailbox_bytes(a.U + 1, a.T);  // lane j owns the states 2j and 2j + 1: U + 1 columns
    if (mbox <= 64 * 1024) {
        if (NW > 1) launch_fill32(a.err, 0u, 4, st);  // one wave: no mailbox, no spin
        hipLaunchKernelGGL(k_ctc_chain<true>, dim3(a.N, 2), dim3(64 * NW), (mbox + 15) / 16 * 16, st, a.lpb, a.lpl, a.alpha,
                           a.beta, a.targets, a.logit_lens, a.target_lens, a.costs, a.logp, a.T, a.U, a.V, a.err);
        if (NW > 1) launch_chain_status(a.err, a.costs, a.logp, a.N, st);  // (NaN in log P: in every gradient of the call too)
    } else {
        hipLaunchKernelGGL(k_ctc_chain<false>, dim3(a.N, 2), dim3(64 * NW), (size_t)2 * NW * 8, st, a.lpb, a.lpl, a.alpha,
                           a.beta, a.targets, a.logit_lens, a.target_lens, a.costs, a.logp, a.T, a.U, a.V, a.err);
    }
    if (!a.grad) return;
    if (a.U > 0) hipLaunchKernelGGL(k_ctc_links, dim3(a.N), dim3(1024), 0, st, a.targets, a.target_lens, a.link, a.U, a.V);
    hipLaunchKernelGGL(k_ctc_grad, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, a.logits, a.targets, a.link, a.logit_lens,
                       a.target_lens, a.denom, a.lpb, a.lpl, a.alpha, a.beta, a.logp, a.weights, a.grad, a.N, a.T, a.U, a.V,
                       a.blank);
}

void launch_ctc_greedy(const float *logits, const int32_t *logit_lens, int N, int T, int V, int blank, int32_t *tokens,
                       int32_t *counts, hipStream_t st)
{
    const long rows = (long)N * T;
    hipLaunchKernelGGL(k_ctc_argmax, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, logits, logit_lens, tokens, N, T, V);
    hipLaunchKernelGGL(k_ctc_collapse, dim3(N), dim3(1024), 0, st, logit_lens, tokens, counts, T, blank);
}
