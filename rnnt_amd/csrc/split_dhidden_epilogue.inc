// split_dhidden_epilogue.inc — the epilogue of the split routes' dHidden kernels (k_dhidden_x3, k_dhidden_x2, k_dhidden_x2r), ONE text
// expanded inside each kernel body (split_dhidden.hpp says why it is no function).  It expects these names in scope:
//   a                X3Args, the kernel's argument block
//   T, U1, H         a.T, a.U1, a.H
//   tl               DhTile: the tile (b, tt, ub, t0, u0) and the utterance's Tb
//   lane, i, half    the lane, lane & 31, lane >> 5
//   F                the piece format (F::dh_unscale)
//   MT, NG, XWAVE    constexpr: M tiles and 128-column groups of acc, and whether two waves (wm = 0, 1) share the tile's t rows
//   acc              f32x16 [MT][4 * NG]
//   mbase, colbase   the first M tile and the first column of acc
//   s_red, wm, wn    XWAVE: float (*)[64][65] over the (free) W ring, [wn][lane][8 u slots x 4 NG columns]; the wave's place
// Accumulator register rr = 8rh + r7 of M tile mbase + mt, column tile q: t row 2(mbase + mt) + rh, u slot 8(r7>>2) + (r7&3) + 4half;
// column colbase + 128(q>>2) + 4i + (q&3) (the dHidden pack interleaves columns by 4: a lane's 4 tiles of a group are 4 adjacent columns).
// XWAVE: the pred rows are requested BEFORE the drain of the over-issued ring loads / DMAs and ride out the G stores' acknowledgements
// with it, then the workgroup joins and wave wm = 1 hands its sums over t to wave wm = 0 through s_red[wn].  Without it (a wave holds
// all 8 t rows) the kernel has drained already.
{
    int colg[NG];
    bool colok[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) { colg[g] = colbase + 128 * g + 4 * i; colok[g] = colg[g] < H; }
    f32x4 pr[8][NG];  // pred rows of this lane's 8 u slots, its NG x 4 columns (zero where u >= U1 or the column >= H)
#pragma unroll
    for (int r7 = 0; r7 < 8; ++r7) {
        const int u = tl.u0 + 8 * (r7 >> 2) + (r7 & 3) + 4 * half;
#pragma unroll
        for (int g = 0; g < NG; ++g)
            pr[r7][g] = (u < U1 && colok[g]) ? *(const f32x4 *)(a.pred + ((long)tl.b * U1 + u) * H + colg[g]) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float unscale = F::dh_unscale(a);
    if (XWAVE) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the over-issued ring loads / DMAs
        __syncthreads();
    }
    const long BTH = (long)a.B * T * H, BUH = (long)a.B * U1 * H;
    f2 psum2[8][2 * NG];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int q = 0; q < 2 * NG; ++q) psum2[k][q] = f2{0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int rh = 0; rh < 2; ++rh) {
            const int t = tl.t0 + 2 * (mbase + mt) + rh;
            f2 esum2[2 * NG];
#pragma unroll
            for (int q = 0; q < 2 * NG; ++q) esum2[q] = f2{0.f, 0.f};
            f32x4 er[NG];
#pragma unroll
            for (int g = 0; g < NG; ++g)
                er[g] = (t < T && colok[g]) ? *(const f32x4 *)(a.enc + (long)tl.b * a.enc_sb + (long)t * a.enc_st + colg[g]) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r7 = 0; r7 < 8; ++r7)
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int qq = 0; qq < 2; ++qq) {  // columns 2qq, 2qq+1 of the group
                        const f2 x = {er[g][2 * qq] + pr[r7][g][2 * qq], er[g][2 * qq + 1] + pr[r7][g][2 * qq + 1]};
                        const f2 av = {acc[mt][g * 4 + 2 * qq][rh * 8 + r7], acc[mt][g * 4 + 2 * qq + 1][rh * 8 + r7]};
                        const f2 d = av * dh_dfac2(x);
                        esum2[g * 2 + qq] += d;
                        psum2[r7][g * 2 + qq] += d;
                    }
            f32x4 es[NG];  // (one vector per group: as a flat array k_dhidden_x2r spills 16 bytes more)
#pragma unroll
            for (int g = 0; g < NG; ++g) es[g] = f32x4{unscale * esum2[2 * g][0], unscale * esum2[2 * g][1], unscale * esum2[2 * g + 1][0], unscale * esum2[2 * g + 1][1]};
#pragma unroll
            for (int g = 0; g < NG; ++g)
#pragma unroll
                for (int q = 0; q < 4; ++q) es[g][q] += __shfl_xor(es[g][q], 32, 64);
            if (half == 0 && t < tl.Tb) {
#pragma unroll
                for (int g = 0; g < NG; ++g)
                    if (colok[g]) *(f32x4 *)(a.slab_enc + (long)tl.ub * BTH + ((long)tl.b * T + t) * H + colg[g]) = es[g];
            }
        }
    float psum[8][4 * NG];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
        for (int q = 0; q < 4 * NG; ++q) psum[k][q] = unscale * psum2[k][q >> 1][q & 1];
    if (XWAVE) {
        if (wm == 1) {
#pragma unroll
            for (int k = 0; k < 8; ++k)
#pragma unroll
                for (int q = 0; q < 4 * NG; ++q) s_red[wn][lane][k * 4 * NG + q] = psum[k][q];
        }
        __syncthreads();
    }
    if (!XWAVE || wm == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int u = tl.u0 + 8 * (k >> 2) + (k & 3) + 4 * half;
            if (u < U1) {
#pragma unroll
                for (int g = 0; g < NG; ++g)
                    if (colok[g]) {
                        f32x4 o;
#pragma unroll
                        for (int q = 0; q < 4; ++q) o[q] = XWAVE ? psum[k][g * 4 + q] + s_red[wn][lane][k * 4 * NG + g * 4 + q] : psum[k][g * 4 + q];
                        *(f32x4 *)(a.slab_pred + (long)tl.tt * BUH + ((long)tl.b * U1 + u) * H + colg[g]) = o;
                    }
            }
        }
    }
}
