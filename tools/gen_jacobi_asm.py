#!/usr/bin/env python3
"""Generates csrc/wm_jacobi_gfx950.inc: the packed one-sided Jacobi of the tile kernels
(wm_tile_math.h: raw_to_pk + jacobi_cols_pk + the final col_norms2_pk) as ONE hand-scheduled gfx950
instruction stream in a single inline-asm statement with pinned registers.

Why not leave it to hipcc (profiles/r02_embed_variants.md): for the C++ form it SLP-packs the rotation's
scalar angle arithmetic into v_pk ops stitched together with v_mov, spends an `s_nop` after most packed
instructions (gfx940 forwarding hazard of VOP3P results), keeps ~140 VGPRs live (3 waves per SIMD) and
spills as soon as the sweep is split into basic blocks.  Here the whole iteration lives in a fixed
register file - B in v[40:103], the column norms in v[104:111], 16 temporaries in v[112:127], the squared column
scales of the untested sweeps' scaled rotations in v[128:135] - so the stream needs 136 VGPRs (three waves per SIMD, where the embed
and extract kernels round it are anyway), and every hazard the stream has is resolved by ORDER:
  * a VOP3P result is never read by the next instruction            (DstSel forwarding hazard, 1 state)
  * a v_rsq_f32 result is never read by the next instruction        (trans-use hazard, 1 state)
  * VCC written by v_cmp is read by v_cndmask two instructions later (VALU SGPR write -> VALU read, 2 states)
The generator checks these three rules on the stream it emits and pads with s_nop where the order
does not already satisfy them (it never needs to inside a rotation).

Same arithmetic as jacobi_rot_pk (two-rsq angle, de Rijk swap, cancellation-free norm update, wave-uniform
skip of a pair that is below the skip threshold in all 64 tiles), same pair order (row-cyclic), same sweep
control (norms recomputed before odd sweeps, convergence test on cos^2 and on the norm move w = |t g|, sweep bound 12).

The untested sweeps (the first min_sweeps - 1) keep the columns scaled, so that a rotation in which no tile of the wave
takes the de Rijk swap costs two packed FMAs per row pair instead of four packed operations (rotation_scaled,
jacobi_rot_scaled_pk); the scales are folded back into B behind the last of them and the tested sweeps are rotation().

Ahead of the first sweep the stream runs the LQ prelude (lq_prelude: B0 = X Q, Householder LQ with greedy row
pivoting applied from the right - about one sweep fewer).  build(lq=False) is the stream without it: never compiled into
a kernel, only interpreted (tools/emu_jacobi_asm.py) as the baseline the prelude is measured against.

A second stream, csrc/wm_jacobi_v_gfx950.inc (build_v), is jacobi_cols_pk_v: the same rotation applied to the
stacked rows of B and V (v[40:103], v[104:167]), every pair tested and rotated, a converged lane leaving the
exec mask - the literal path of rank-deficient tiles and the watermark-side SVD.

A third, csrc/wm_jacobi_sigma_gfx950.inc (build(sigma_only=True)), is the V-free stream for the callers that take only
the singular values: the columns stay scaled through the tested sweeps too and are never folded back.  It is not
committed (write_sigma() says why): `--write` and the package's build() generate it.

    python tools/gen_jacobi_asm.py --write  # rewrites the .inc files next to the kernels where they differ
"""
import os
import struct
import sys

MAX_SWEEPS = 12
MOVE2 = 1e-6          # JAC_MOVE2 of wm_tile_math.h


class Lay:
    """Register file of one stream: B at v[a0 ..], optionally V at v[v0 ..], norms, 16 temporaries at v[t ..]."""

    def __init__(self, a0, n0, t, v0=None, vn0=None, w0=None):
        self.A0, self.N0, self.T, self.V0, self.VN0, self.W0 = a0, n0, t, v0, vn0, w0
        pr = lambda k: f"v[{t + k}:{t + k + 1}]"
        self.GV, self.T1, self.T2, self.CS, self.T3 = pr(0), pr(2), pr(4), pr(6), pr(14)
        self.GVl, self.GVh, self.C, self.S = f"v{t}", f"v{t + 1}", f"v{t + 6}", f"v{t + 7}"
        (self.g, self.gg, self.ab, self.tau, self.ta, self.t1, self.ih, self.x) = (f"v{t + k}" for k in range(8, 16))

    def A(self, rp, c, base=None):
        b = (self.A0 if base is None else base) + 2 * (8 * rp + c)
        return f"v[{b}:{b + 1}]"

    def V(self, rp, c):
        return self.A(rp, c, self.V0)

    def Alo(self, rp, c):
        return f"v{self.A0 + 2 * (8 * rp + c)}"

    def Ahi(self, rp, c):
        return f"v{self.A0 + 2 * (8 * rp + c) + 1}"

    def N(self, c, base=None):
        return f"v{(self.N0 if base is None else base) + c}"

    def W(self, c):
        return f"v{self.W0 + c}"

    def WP(self, c):
        b = self.W0 + 2 * (c >> 1)
        return f"v[{b}:{b + 1}]"


# the V-free stream (embed / sigma kernels): B in v[40:103], n2 in v[104:111], temporaries v[112:127], the squared
# column scales of the scaled rotations in v[128:135]
LAY = Lay(40, 104, 112, w0=128)
A0, N0, T = LAY.A0, LAY.N0, LAY.T
# the stream with V (fallback embed, watermark-side SVD): B v[40:103], V v[104:167], |b|^2 v[168:175], |v|^2 v[176:183],
# temporaries v[184:199]
LAY_V = Lay(40, 168, 184, v0=104, vn0=176)
# SGPRs (clobbered): mask, sweep counter, constants
M, SW, EPS, CONV, SKIPC, MINSW, SKIPFROM = "s[80:81]", "s82", "s83", "s84", "s85", "s86", "s87"
TMPM, NOSKIP, TMPS = "s[88:89]", "s[90:91]", "s98"
LQ_STEPS = 7            # reflectors of the LQ prelude (5 / 6 / 7: 4.45 / 4.30 / 4.15 embed sweeps per wave on noise tiles)
LQ_T, LQ_FOUND, LQ_M = "s[92:93]", "s[94:95]", "s[96:97]"   # LQ prelude: compare result, rows matched so far, this row's one-hot
DEFI_FROM = 6           # from this many sweeps on, a lane whose tile is rank deficient no longer keeps its wave iterating
SIGMA_FOLD_AT = 6       # sigma-only stream: the 0-based sweep ahead of whose norms the scales are folded into B, once
SAVE = "s[88:89]"       # with-V stream: the caller's exec mask (TMPM / NOSKIP are unused there)


class Stream:
    """Instruction list with the three ordering rules checked as it grows."""

    def __init__(self):
        self.lines = []
        self.hist = []          # (kind, set of written regs) of the last few VALU-slot instructions

    @staticmethod
    def regs(op):
        op = op.strip().lstrip("|-").rstrip("|")
        if op.startswith("v["):
            a, b = op[2:-1].split(":")
            return {f"v{i}" for i in range(int(a), int(b) + 1)}
        if op.startswith("v") and op[1:].isdigit():
            return {op}
        if op == "vcc":
            return {"vcc"}
        if op.startswith("s["):
            a, b = op[2:-1].split(":")
            return {f"s{i}" for i in range(int(a), int(b) + 1)}
        return set()

    def emit(self, text, kind="valu", reads_vcc=False):
        if text.endswith(":") or kind in ("salu", "label"):
            self.lines.append(text)
            if kind == "salu":
                self.hist.append(("salu", set()))
            return
        mn, rest = text.split(None, 1)
        ops = [o.strip() for o in rest.split(" op_sel")[0].split(" neg_")[0].split(",")]
        dst, srcs = ops[0], ops[1:]
        read = set()
        for s_ in srcs:
            read |= self.regs(s_)
        if reads_vcc:
            read.add("vcc")
        need = 0
        for d, (k, w) in enumerate(reversed(self.hist[-3:]), start=1):
            if not (w & read):
                continue
            if k in ("pk", "trans") and d < 2:
                need = max(need, 2 - d)
            if k == "vcmp" and mn.startswith("v_") and d < 3:      # (w & read) holds vcc or the compare's SGPR pair
                need = max(need, 3 - d)
        if need:
            self.lines.append(f"s_nop {need - 1}")
            for _ in range(need):
                self.hist.append(("nop", set()))
        k = "pk" if mn.startswith(("v_pk_", "v_dot4_")) else "trans" if mn.startswith(("v_rsq", "v_rcp")) else "vcmp" if mn.startswith("v_cmp") else "valu"
        self.lines.append(text)
        self.hist.append((k, self.regs(dst) | ({"vcc"} if k == "vcmp" and dst == "vcc" else set())))

    def nops(self):
        return sum(1 for ln in self.lines if ln.startswith("s_nop"))


def col_norms(st, L=LAY, of_v=False):
    """n2[c] = sum over rows of a[.][c]^2: four independent chains at a time (no packed result is read
    by the instruction after its producer).  of_v: the norms of V's columns into vn2."""
    tmps = [L.GV, L.T1, L.T2, L.CS]
    mat = (lambda rp, c: L.V(rp, c)) if of_v else (lambda rp, c: L.A(rp, c))
    nb = L.VN0 if of_v else L.N0
    for c0 in (0, 4):
        for i in range(4):
            st.emit(f"v_pk_mul_f32 {tmps[i]}, {mat(0, c0 + i)}, {mat(0, c0 + i)}")
        for rp in (1, 2, 3):
            for i in range(4):
                st.emit(f"v_pk_fma_f32 {tmps[i]}, {mat(rp, c0 + i)}, {mat(rp, c0 + i)}, {tmps[i]}")
        for i in range(4):
            lo = tmps[i][2:-1].split(":")[0]
            st.emit(f"v_add_f32_e32 {L.N(c0 + i, nb)}, v{lo}, v{int(lo) + 1}")


def rotation(st, p, q, uid, plain=False, L=LAY, with_v=False, move_test=True):
    """One Jacobi rotation of columns p < q (jacobi_rot_pk<CHECK, SKIP>); plain: no convergence test, no skip
    (the sweeps that can never be the last one); with_v: tested, never skipped, V's columns rotated too
    (jacobi_rot_pk_v<1>); move_test: the tested rotation also reports a norm move above MOVE2."""
    A, N = L.A, L.N
    GV, T1, T2, CS, T3, GVl, GVh, C, S = L.GV, L.T1, L.T2, L.CS, L.T3, L.GVl, L.GVh, L.C, L.S
    g, gg, ab, tau, ta, t1, ih, x = L.g, L.gg, L.ab, L.tau, L.ta, L.t1, L.ih, L.x
    Np, Nq = N(p), N(q)
    st.emit(f"v_pk_mul_f32 {GV}, {A(0, p)}, {A(0, q)}")
    st.emit(f"v_max_f32_e32 {ab}, {Np}, {Nq}" if plain else f"v_mul_f32_e32 {ab}, {Np}, {Nq}")
    st.emit(f"v_pk_fma_f32 {GV}, {A(1, p)}, {A(1, q)}, {GV}")
    st.emit(f"v_sub_f32_e32 {tau}, {Nq}, {Np}")                       # tau = be - al
    st.emit(f"v_pk_fma_f32 {GV}, {A(2, p)}, {A(2, q)}, {GV}")
    st.emit(f"v_add_f32_e64 {ta}, |{tau}|, {EPS}")                     # |tau| + 1e-18
    st.emit(f"v_pk_fma_f32 {GV}, {A(3, p)}, {A(3, q)}, {GV}")
    st.emit(f"v_mul_f32_e32 {t1}, {ta}, {ta}")
    st.emit(f"v_add_f32_e32 {g}, {GVl}, {GVh}")                        # g = a_p . a_q
    if plain:
        st.emit(f"v_mul_f32_e32 {gg}, {g}, {g}")
    elif with_v:
        st.emit(f"v_mul_f32_e32 {x}, {CONV}, {ab}")
        st.emit(f"v_mul_f32_e32 {gg}, {g}, {g}")
        st.emit(f"v_cmp_gt_f32_e32 vcc, {gg}, {x}")                    # notconv |= g^2 > conv2 al be (active lanes only)
        st.emit(f"s_or_b64 {M}, {M}, vcc", kind="salu")
    else:
        st.emit(f"v_mul_f32_e32 {x}, {CONV}, {ab}")
        st.emit(f"v_mul_f32_e32 {gg}, {g}, {g}")
        st.emit(f"v_mul_f32_e32 {ih}, {SKIPC}, {ab}")
        st.emit(f"v_cmp_gt_f32_e32 vcc, {gg}, {x}")                    # notconv |= g^2 > conv2 al be
        st.emit(f"s_or_b64 {M}, {M}, vcc", kind="salu")
        st.emit(f"v_cmp_gt_f32_e32 vcc, {gg}, {ih}")                   # any tile above the skip threshold ...
        st.emit(f"s_or_b64 {TMPM}, vcc, {NOSKIP}", kind="salu")        # ... or a sweep that rotates every pair (SCC = result != 0)
        st.emit(f"s_cbranch_scc0 .Lwmj_skip_{uid}_%=", kind="salu")
    st.emit(f"v_fma_f32 {t1}, {gg}, 4.0, {t1}")                        # h^2 = tau^2 + 4 g^2
    st.emit(f"v_rsq_f32_e32 {ih}, {t1}")                               # 1/h
    st.emit(f"v_mul_f32_e32 {x}, 0.5, {ta}")
    st.emit(f"v_fma_f32 {x}, {x}, {ih}, 0.5")                          # cos^2 in [0.5, 1]
    st.emit(f"v_rsq_f32_e32 {t1}, {x}")                                # rx
    st.emit(f"v_mul_f32_e32 {GVh}, {g}, {ih}")
    st.emit(f"v_mul_f32_e32 {GVl}, {x}, {t1}")                         # c0 = cos
    st.emit(f"v_mul_f32_e32 {GVh}, {GVh}, {t1}")                       # s0 = sin * sign(g)
    st.emit(f"v_cmp_lt_f32_e32 vcc, 0, {tau}")                         # de Rijk: |a_q| > |a_p| -> swap roles
    st.emit(f"v_mul_f32_e32 {gg}, {GVh}, {t1}")                        # t = s0 / c0 ...
    if plain:
        st.emit(f"v_min_f32_e32 {ta}, {Np}, {Nq}")                     # (ta is dead after cos^2)
    else:
        st.emit(f"v_max_f32_e32 {ab}, {Np}, {Nq}")
    st.emit(f"v_cndmask_b32_e32 {C}, {GVl}, {GVh}, vcc", reads_vcc=True)   # C = sw ? s0 : c0
    st.emit(f"v_cndmask_b32_e32 {S}, {GVh}, {GVl}, vcc", reads_vcc=True)   # S = sw ? c0 : s0
    st.emit(f"v_mul_f32_e32 {gg}, {gg}, {g}")                          # ... w = t g  (|w| below)
    if not plain:
        st.emit(f"v_min_f32_e32 {ta}, {Np}, {Nq}")
    if not plain and not with_v and move_test:
        # notconv |= w^2 > move2 max(al, be) n2[0]: the rotation moved a squared singular value by more than
        # sqrt(move2) s_1 s_p (w is |g| for a near-degenerate pair, g^2 / gap for a separated one)
        st.emit(f"v_mul_f32_e32 {x}, {gg}, {gg}")
        st.emit(f"v_mul_f32_e32 {ih}, {f32_literal(MOVE2)}, {ab}")
        st.emit(f"v_mul_f32_e32 {ih}, {ih}, {N(0)}")
        st.emit(f"v_cmp_gt_f32_e32 vcc, {x}, {ih}")
        st.emit(f"s_or_b64 {M}, {M}, vcc", kind="salu")
    st.emit(f"v_add_f32_e64 {Np}, {ab}, |{gg}|")                       # larger norm grows by |t g|
    st.emit(f"v_sub_f32_e64 {Nq}, {ta}, |{gg}|")
    # columns: a_p <- C a_p + S a_q ; a_q <- C a_q - S a_p   (C, S broadcast from the halves of CS by op_sel)
    mats = [L.A] + ([L.V] if with_v else [])
    for mat in mats:
        for rp0 in (0, 2):
            tt = ((T1, T2), (GV, T3))
            for i in (0, 1):
                rp = rp0 + i
                st.emit(f"v_pk_mul_f32 {tt[i][0]}, {CS}, {mat(rp, q)} op_sel:[1,0]")
                st.emit(f"v_pk_mul_f32 {tt[i][1]}, {CS}, {mat(rp, p)} op_sel:[1,0]")
            for i in (0, 1):
                rp = rp0 + i
                st.emit(f"v_pk_fma_f32 {mat(rp, p)}, {CS}, {mat(rp, p)}, {tt[i][0]} op_sel_hi:[0,1,1]")
                st.emit(f"v_pk_fma_f32 {mat(rp, q)}, {CS}, {mat(rp, q)}, {tt[i][1]} op_sel_hi:[0,1,1] neg_lo:[0,0,1] neg_hi:[0,0,1]")
    if not plain and not with_v:
        st.emit(f".Lwmj_skip_{uid}_%=:", kind="label")
        st.hist.append(("nop", set()))       # a taken branch lands here: nothing before it may be assumed


def rotation_scaled(st, p, q, uid, L=LAY, swapfree=True, rcp=False, tested=False, move_test=True):
    """rotation(plain=True) on SCALED columns a_c = sqrt(w_c) at_c, for the untested sweeps of the V-free stream: B's
    registers hold at_c, L.W(c) the squared scale w_c (jacobi_rot_scaled_pk).  Where no tile of the wave takes the de
    Rijk swap (tau <= 0 in all 64 lanes) the update is two packed FMAs per row pair and no product,
        at_p += t_p at_q ;  at_q -= t_q at_p'         (a_p' = c (a_p + t a_q),  a_q' = a_q / c - t a_p')
        t_p = (gt / h) w_q / c^2,  t_q = (gt / h) w_p,   w_p *= c^2,  w_q /= c^2,      gt = at_p . at_q
    and needs no reciprocal or root of a scale: c^2 and 1 / c^2 are what the angle's two v_rsq_f32 deliver anyway.
    g^2 = gt^2 w_p w_q feeds the angle, the norm move is |t g| = g^2 / (h c^2); the tracked norms n2 are the TRUE ones.
    Behind the LQ prelude the columns arrive graded: a swap is wanted at about 8 of the first sweep's 28 pairs, 3 of the
    second's and none later (tools/conv_study.cpp 4).  Where any lane swaps, the wave takes rotation()'s four-product
    update with the scale ratios folded into its coefficients, at_p' = C at_p + S (d_q / d_p) at_q, at_q' = C at_q -
    S (d_p / d_q) at_p (one more v_rsq_f32, of w_p w_q); the scales stay as they are.
    Scale range: c^2 is in [0.5, 1], a rotation leaves the product of the eight w at 1, and a column meets 7 rotations
    in each of at most 3 untested sweeps: 2^-21 <= w <= 2^21, no rescaling.  (The study's tiles stay within [0.2, 5].)
    swapfree: the swap-free path runs only where tau = n2[q] - n2[p] <= 0 in every lane, so there max(n2[p], n2[q]) IS
    n2[p] and the min IS n2[q], bit for bit: the two norms are updated in place and the max / min are left to the swap
    branch (two scalar instructions fewer per swap-free rotation, the same bits).  swapfree=False is the body as it was,
    max and min ahead of the branch: never compiled, only interpreted as the baseline the new body is held against.
    rcp: 1 / c^2 is one v_rcp_f32 of c^2 where it is v_rsq_f32 and a square (one scalar instruction fewer on the
    swap-free path, the last bit of a scale may differ); the swap branch, which needs 1 / c itself, takes its own
    v_rsq_f32.  The sigma-only stream has it; the stream that hands out B does not (build()).
    tested (the sigma-only stream, whose columns stay scaled to the end): rotation()'s convergence, skip and norm-move
    tests ahead of the same update, on the true g^2 = gt^2 w_p w_q and the true norms.
    Scale range with tested sweeps: 2^-7 <= w'/w <= 2^7 per sweep (seven rotations, c^2 in [0.5, 1]).  Up to the sweep
    bound of 12 that would be 2^+-84 and the product w_p w_q of a rotation could leave the float range, so the
    sigma-only stream folds the scales into B once, where the 7th sweep recomputes its norms (build(sigma_only=True)):
    2^-42 <= w <= 2^42 on either side of it, w_p w_q and gt w_p w_q = g sqrt(w_p w_q) <= 2^21 2^42 stay normal floats.
    (A wave gets there only with rank-deficient tiles; the study's tiles stay within [0.2, 5] throughout.)"""
    assert swapfree or not tested
    A, N, W = L.A, L.N, L.W
    GV, T1, T2, CS, T3, GVl, GVh, C, S = L.GV, L.T1, L.T2, L.CS, L.T3, L.GVl, L.GVh, L.C, L.S
    g, gg, ab, tau, ta, t1, ih, x = L.g, L.gg, L.ab, L.tau, L.ta, L.t1, L.ih, L.x
    P89 = f"v[{L.T + 8}:{L.T + 9}]"                                     # (g, gg): free once s0 and the norms are there
    Np, Nq = N(p), N(q)
    # the dot product's packed chain, a scalar instruction between two links (a packed result is never read by the
    # next instruction); without the max, the product of the scales is what parts the last link from its sum
    fill = [f"v_sub_f32_e32 {tau}, {Nq}, {Np}",                        # tau = be - al
            f"v_add_f32_e64 {ta}, |{tau}|, {EPS}",                     # |tau| + 1e-18 (the eps: tau = g = 0 -> cos^2 = 1, not 0.5)
            f"v_mul_f32_e32 {t1}, {ta}, {ta}",
            f"v_mul_f32_e32 {x}, {W(p)}, {W(q)}"]
    dot = f"v_add_f32_e32 {g}, {GVl}, {GVh}"                           # gt = at_p . at_q
    tail = [fill[3], dot] if swapfree else [dot, fill[3]]
    fill = fill[:3] if swapfree else [f"v_max_f32_e32 {ab}, {Np}, {Nq}"] + fill[:3]
    if tested:
        tail = [f"v_mul_f32_e32 {ab}, {Np}, {Nq}"] + tail
    st.emit(f"v_pk_mul_f32 {GV}, {A(0, p)}, {A(0, q)}")
    for rp in (1, 2, 3):
        st.emit(fill[rp - 1])
        st.emit(f"v_pk_fma_f32 {GV}, {A(rp, p)}, {A(rp, q)}, {GV}")
    for ln in fill[3:] + tail:
        st.emit(ln)
    st.emit(f"v_mul_f32_e32 {gg}, {g}, {x}")
    st.emit(f"v_mul_f32_e32 {gg}, {gg}, {g}")                          # g^2 = (gt w_p w_q) gt
    if tested:
        st.emit(f"v_mul_f32_e32 {x}, {CONV}, {ab}")
        st.emit(f"v_mul_f32_e32 {ih}, {SKIPC}, {ab}")
        st.emit(f"v_cmp_gt_f32_e32 vcc, {gg}, {x}")                    # notconv |= g^2 > conv2 al be
        st.emit(f"s_or_b64 {M}, {M}, vcc", kind="salu")
        st.emit(f"v_cmp_gt_f32_e32 vcc, {gg}, {ih}")                   # any tile above the skip threshold ...
        st.emit(f"s_or_b64 {TMPM}, vcc, {NOSKIP}", kind="salu")        # ... or a sweep that rotates every pair (SCC = result != 0)
        st.emit(f"s_cbranch_scc0 .Lwmj_rot_{uid}_%=", kind="salu")
    st.emit(f"v_fma_f32 {t1}, {gg}, 4.0, {t1}")                        # h^2 = tau^2 + 4 g^2
    st.emit(f"v_rsq_f32_e32 {ih}, {t1}")                               # 1/h
    st.emit(f"v_mul_f32_e32 {x}, 0.5, {ta}")
    st.emit(f"v_fma_f32 {x}, {x}, {ih}, 0.5")                          # cos^2 in [0.5, 1]
    st.emit(f"v_rcp_f32_e32 {t1}, {x}" if rcp else                     # 1 / cos^2
            f"v_rsq_f32_e32 {t1}, {x}")                                # rx = 1 / cos
    st.emit(f"v_mul_f32_e32 {GVh}, {g}, {ih}")                         # u = gt / h
    st.emit(f"v_cmp_lt_f32_e32 vcc, 0, {tau}")                         # de Rijk: does any tile of the wave want the swap?
    st.emit(f"v_mul_f32_e32 {gg}, {gg}, {ih}")                         # g^2 / h
    maxmin = [f"v_max_f32_e32 {ab}, {Np}, {Nq}", f"v_min_f32_e32 {ta}, {Np}, {Nq}"]     # (ta is dead after cos^2)
    big, small = (Np, Nq) if swapfree else (ab, ta)                    # no lane swaps: n2[p] is the larger norm in every lane
    if not swapfree:
        st.emit(maxmin[1])
    st.emit(f"s_cbranch_vccnz .Lwmj_swap_{uid}_%=", kind="salu")
    # -- no lane swaps
    if not rcp:
        st.emit(f"v_mul_f32_e32 {t1}, {t1}, {t1}")                     # 1 / cos^2
    st.emit(f"v_mul_f32_e32 {S}, {GVh}, {W(p)}")                       # t_q = u w_p
    st.emit(f"v_mul_f32_e32 {GVh}, {GVh}, {t1}")
    st.emit(f"v_mul_f32_e32 {gg}, {gg}, {t1}")                         # w = g^2 / (h cos^2) = |t g|
    st.emit(f"v_mul_f32_e32 {W(p)}, {W(p)}, {x}")
    st.emit(f"v_mul_f32_e32 {C}, {GVh}, {W(q)}")                       # t_p = u w_q / cos^2
    st.emit(f"v_mul_f32_e32 {W(q)}, {W(q)}, {t1}")
    if tested and move_test:                                           # notconv |= w^2 > move2 n2[p] n2[0] (rotation())
        st.emit(f"v_mul_f32_e32 {ih}, {f32_literal(MOVE2)}, {Np}")
        st.emit(f"v_mul_f32_e32 {x}, {gg}, {gg}")
        st.emit(f"v_mul_f32_e32 {ih}, {ih}, {N(0)}")
        st.emit(f"v_cmp_gt_f32_e32 vcc, {x}, {ih}")
        st.emit(f"s_or_b64 {M}, {M}, vcc", kind="salu")
    st.emit(f"v_add_f32_e64 {Np}, {big}, |{gg}|")                      # larger norm grows by |t g|
    st.emit(f"v_sub_f32_e64 {Nq}, {small}, |{gg}|")
    for rp in range(4):
        st.emit(f"v_pk_fma_f32 {A(rp, p)}, {CS}, {A(rp, q)}, {A(rp, p)} op_sel_hi:[0,1,1]")
    for rp in range(4):
        st.emit(f"v_pk_fma_f32 {A(rp, q)}, {CS}, {A(rp, p)}, {A(rp, q)} op_sel:[1,0,0] neg_lo:[1,0,0] neg_hi:[1,0,0]")
    st.emit(f"s_branch .Lwmj_rot_{uid}_%=", kind="salu")
    # -- some lane swaps: rotation()'s update on the scaled columns
    st.emit(f".Lwmj_swap_{uid}_%=:", kind="label")
    st.hist.append(("nop", set()))
    if rcp:
        st.emit(f"v_rsq_f32_e32 {t1}, {x}")                            # rx = 1 / cos
    if swapfree:
        st.emit(maxmin[0])
        st.emit(maxmin[1])
    st.emit(f"v_mul_f32_e32 {ih}, {W(p)}, {W(q)}")
    st.emit(f"v_mul_f32_e32 {GVl}, {x}, {t1}")                         # c0 = cos
    st.emit(f"v_rsq_f32_e32 {x}, {ih}")                                # 1 / (d_p d_q)
    st.emit(f"v_mul_f32_e32 {gg}, {gg}, {t1}")
    st.emit(f"v_mul_f32_e32 {GVh}, {GVh}, {t1}")
    st.emit(f"v_mul_f32_e32 {gg}, {gg}, {t1}")                         # w
    st.emit(f"v_mul_f32_e32 {ih}, {ih}, {x}")                          # d_p d_q
    if tested and move_test:                                           # (tau is dead: VCC holds the swap; n2[0] as it was)
        st.emit(f"v_mul_f32_e32 {tau}, {gg}, {gg}")
        st.emit(f"v_sub_f32_e64 {Nq}, {ta}, |{gg}|")
        st.emit(f"v_mul_f32_e32 {ta}, {f32_literal(MOVE2)}, {ab}")
        st.emit(f"v_mul_f32_e32 {ta}, {ta}, {N(0)}")
        st.emit(f"v_add_f32_e64 {Np}, {ab}, |{gg}|")
    else:
        st.emit(f"v_add_f32_e64 {Np}, {ab}, |{gg}|")
        st.emit(f"v_sub_f32_e64 {Nq}, {ta}, |{gg}|")
    st.emit(f"v_mul_f32_e32 {GVh}, {GVh}, {ih}")                       # s0 = u d_p d_q / cos = sin * sign(g)
    st.emit(f"v_mul_f32_e32 {ih}, {W(q)}, {x}")                        # d_q / d_p
    st.emit(f"v_mul_f32_e32 {x}, {W(p)}, {x}")                         # d_p / d_q
    st.emit(f"v_cndmask_b32_e32 {t1}, {GVh}, {GVl}, vcc", reads_vcc=True)    # S = sw ? c0 : s0
    st.emit(f"v_cndmask_b32_e32 {C}, {GVl}, {GVh}, vcc", reads_vcc=True)     # C = sw ? s0 : c0, in both pairs
    st.emit(f"v_cndmask_b32_e32 {g}, {GVl}, {GVh}, vcc", reads_vcc=True)
    st.emit(f"v_mul_f32_e32 {S}, {t1}, {ih}")                          # CS = (C, S d_q / d_p): the new at_p
    st.emit(f"v_mul_f32_e32 {gg}, {t1}, {x}")                          # P89 = (C, S d_p / d_q): the new at_q
    if tested and move_test:
        st.emit(f"v_cmp_gt_f32_e32 vcc, {tau}, {ta}")                  # notconv |= w^2 > move2 max(al, be) n2[0]
        st.emit(f"s_or_b64 {M}, {M}, vcc", kind="salu")
    for rp0 in (0, 2):
        tt = ((T1, T2), (GV, T3))
        for i in (0, 1):
            rp = rp0 + i
            st.emit(f"v_pk_mul_f32 {tt[i][0]}, {CS}, {A(rp, q)} op_sel:[1,0]")
            st.emit(f"v_pk_mul_f32 {tt[i][1]}, {P89}, {A(rp, p)} op_sel:[1,0]")
        for i in (0, 1):
            rp = rp0 + i
            st.emit(f"v_pk_fma_f32 {A(rp, p)}, {CS}, {A(rp, p)}, {tt[i][0]} op_sel_hi:[0,1,1]")
            st.emit(f"v_pk_fma_f32 {A(rp, q)}, {P89}, {A(rp, q)}, {tt[i][1]} op_sel_hi:[0,1,1] neg_lo:[0,0,1] neg_hi:[0,0,1]")
    st.emit(f".Lwmj_rot_{uid}_%=:", kind="label")
    st.hist.append(("nop", set()))       # a taken branch lands here: nothing before it may be assumed


def scale_norms(st, L=LAY):
    """the squared norms col_norms() took from the scaled columns, made true: n2[c] *= w_c (w_c = 1 once the scales are
    folded back)"""
    for c in range(8):
        st.emit(f"v_mul_f32_e32 {L.N(c)}, {L.N(c)}, {L.W(c)}")


def fold_scales(st, L=LAY):
    """B's registers become the true columns again, a_c = sqrt(w_c) at_c, and the scales 1: once, behind the last
    untested sweep"""
    for c in range(8):
        st.emit(f"v_rsq_f32_e32 v{L.T + c}, {L.W(c)}")
    for c in range(8):
        st.emit(f"v_mul_f32_e32 {L.W(c)}, {L.W(c)}, v{L.T + c}")
    for c in range(8):
        h = c & 1
        for rp in range(4):
            st.emit(f"v_pk_mul_f32 {L.A(rp, c)}, {L.WP(c)}, {L.A(rp, c)} op_sel:[{h},0] op_sel_hi:[{h},1]")
    for c in range(8):
        st.emit(f"v_mov_b32_e32 {L.W(c)}, 1.0")


def f32_literal(x):
    return f"0x{struct.unpack('<I', struct.pack('<f', x))[0]:08x}"


def lq_prelude(st, L=LAY, byte_norms=True):
    """B0 = X Q: Householder LQ of the tile with greedy row pivoting, reflectors applied from the RIGHT (lq_prelude_pk of
    wm_tile_math.h).  Step k = 0 .. 6: the row not yet used with the largest |x[k:]|^2 is the pivot; the reflector
    H = I - vh vh^T (vh = (x + sign(x_k) |x| e_k) sqrt(2 / v^T v), columns k .. 7) zeroes its entries k+1 .. 7 and is
    applied to all eight rows.  The column Gram matrix of B0 is that of the row-pivoted R^T - one QR-algorithm step
    further on than X's - and the row permutation never has to be applied.  B0 = X * (orthogonal), so everything
    downstream of the sweeps is unchanged.  A wrong pivot (ties, cancellation in the downdated norms) only costs
    convergence; a zero row gives vh = 0.
    Registers, all free before the first sweep: vh / the selected row in v[N0 : N0+7] (column c in half c & 1 of pair
    c >> 1), W = A vh in v[T : T+7], the trailing row norms in v[T+8 : T+15] (row r in v[T+8+r]); scalars of a step in
    W's registers before W is formed.  The one-hot row masks are made exclusive on the scalar unit (first match wins)
    and read by v_cndmask from SGPRs the SALU wrote.
    byte_norms: the eight |row|^2 come from the raw row words, which are still live here: v_dot4_u32_u8 of the low word
    with itself, of the high word on top of it, v_cvt_f32_u32 - 24 instructions for the 32 packed ones of the float
    chain, and the same bits, since every partial sum of that chain is an integer <= 8 * 255^2 < 2^24 and so exact.
    byte_norms=False is the packed chain: never compiled, only interpreted as the baseline."""
    e = st.emit
    X = lambda c: f"v{L.N0 + c}"
    XP = lambda c: f"v[{L.N0 + 2 * (c >> 1)}:{L.N0 + 2 * (c >> 1) + 1}]"
    W = lambda rp: f"v[{L.T + 2 * rp}:{L.T + 2 * rp + 1}]"
    RNP = lambda rp: f"v[{L.T + 8 + 2 * rp}:{L.T + 9 + 2 * rp}]"
    RN = lambda r: f"v{L.T + 8 + r}"
    row = lambda r, c: L.Alo(r >> 1, c) if (r & 1) == 0 else L.Ahi(r >> 1, c)
    m, neg, t2, nx2, rr, nrm, vk, sb = (f"v{L.T + i}" for i in range(8))
    tiny = f32_literal(1e-36)
    if byte_norms:                                       # |row|^2 of all eight rows, in integers
        for r in range(8):
            e(f"v_dot4_u32_u8 {RN(r)}, %[lo{r}], %[lo{r}], 0")
        for r in range(8):
            e(f"v_dot4_u32_u8 {RN(r)}, %[hi{r}], %[hi{r}], {RN(r)}")
        for r in range(8):
            e(f"v_cvt_f32_u32_e32 {RN(r)}, {RN(r)}")
    for c in range(0 if byte_norms else 8):              # the same in floats: four packed chains
        for rp in range(4):
            e(f"v_pk_mul_f32 {RNP(rp)}, {L.A(rp, c)}, {L.A(rp, c)}" if c == 0 else
              f"v_pk_fma_f32 {RNP(rp)}, {L.A(rp, c)}, {L.A(rp, c)}, {RNP(rp)}")
    for k in range(LQ_STEPS):
        cols = range(k, 8)
        e(f"v_max3_f32 {m}, {RN(0)}, {RN(1)}, {RN(2)}")
        e(f"v_max3_f32 {neg}, {RN(3)}, {RN(4)}, {RN(5)}")
        e(f"v_max3_f32 {m}, {RN(6)}, {RN(7)}, {m}")
        e(f"s_mov_b64 {LQ_FOUND}, 0", kind="salu")
        e(f"v_max_f32_e32 {m}, {m}, {neg}")
        e(f"v_mov_b32_e32 {neg}, {f32_literal(-1e30)}")   # a used row never wins again
        for r in range(8):
            e(f"v_cmp_eq_f32_e64 {LQ_T}, {RN(r)}, {m}")
            e(f"s_andn2_b64 {LQ_M}, {LQ_T}, {LQ_FOUND}", kind="salu")
            e(f"s_or_b64 {LQ_FOUND}, {LQ_FOUND}, {LQ_T}", kind="salu")
            if r < 7:                                    # (row 7's own mark: below, where it keeps v_rsq and its use apart)
                e(f"v_cndmask_b32_e64 {RN(r)}, {RN(r)}, {neg}, {LQ_M}")
            if r:
                for c in cols:                           # x = the pivot row's entries k .. 7 (row 0 unless another matched)
                    e(f"v_cndmask_b32_e64 {X(c)}, {row(0, c) if r == 1 else X(c)}, {row(r, c)}, {LQ_M}")
        e(f"v_mul_f32_e32 {t2}, {X(7)}, {X(7)}")
        for c in range(6, k, -1):
            e(f"v_fma_f32 {t2}, {X(c)}, {X(c)}, {t2}")    # |x[k+1:]|^2
        e(f"v_fma_f32 {nx2}, {X(k)}, {X(k)}, {t2}")
        e(f"v_max_f32_e32 {rr}, {tiny}, {nx2}")
        e(f"v_rsq_f32_e32 {rr}, {rr}")
        e(f"v_mov_b32_e32 {vk}, 0x7fffffff")
        e(f"v_mul_f32_e32 {nrm}, {nx2}, {rr}")            # |x| (0 for a zero row)
        e(f"v_bfi_b32 {nrm}, {vk}, {nrm}, {X(k)}")        # sign(x_k) |x|
        e(f"v_add_f32_e32 {vk}, {X(k)}, {nrm}")           # v_k = x_k + sign(x_k) |x|: no cancellation
        e(f"v_fma_f32 {t2}, {vk}, {vk}, {t2}")            # v^T v
        e(f"v_mul_f32_e32 {t2}, 0.5, {t2}")
        e(f"v_max_f32_e32 {t2}, {tiny}, {t2}")
        e(f"v_rsq_f32_e32 {sb}, {t2}")                    # sqrt(2 / v^T v)
        e(f"v_cndmask_b32_e64 {RN(7)}, {RN(7)}, {neg}, {LQ_M}")   # row 7 used, if it is the pivot ({LQ_M} is still its one-hot)
        for c in cols:
            e(f"v_mul_f32_e32 {X(c)}, {vk if c == k else X(c)}, {sb}")      # vh
        for c in cols:                                   # W = A vh (both rows of a pair at once)
            h = c & 1
            for rp in range(4):
                e(f"v_pk_mul_f32 {W(rp)}, {XP(c)}, {L.A(rp, c)} op_sel:[{h},0] op_sel_hi:[{h},1]" if c == k else
                  f"v_pk_fma_f32 {W(rp)}, {XP(c)}, {L.A(rp, c)}, {W(rp)} op_sel:[{h},0,0] op_sel_hi:[{h},1,1]")
        for c in cols:                                   # A <- A - W vh^T
            h = c & 1
            for rp in range(4):
                e(f"v_pk_fma_f32 {L.A(rp, c)}, {XP(c)}, {W(rp)}, {L.A(rp, c)} op_sel:[{h},0,0] op_sel_hi:[{h},1,1] "
                  f"neg_lo:[0,1,0] neg_hi:[0,1,0]")
        if k < LQ_STEPS - 1:
            for rp in range(4):                          # trailing norms lose column k
                e(f"v_pk_fma_f32 {RNP(rp)}, {L.A(rp, k)}, {L.A(rp, k)}, {RNP(rp)} neg_lo:[1,0,0] neg_hi:[1,0,0]")


def eps_literal():
    return struct.unpack("<I", struct.pack("<f", 1e-18))[0]  # keeps 0/0 out; its square (1e-36) is a normal float


def build(move_test=True, lq=True, scaled=True, swapfree=True, byte_norms=None, rcp=None, sigma_only=False):
    """lq=False: no LQ prelude; move_test=False: the tested sweeps stop on cos^2 alone, as they did before the LQ prelude (what the emulator
    measures the prelude against); scaled=False: every pair takes rotation() on unscaled columns (what the scaled
    rotations are measured against); swapfree=False: the scaled rotations with max / min of the two norms ahead of the
    branch (what the in-place norm update of the swap-free path is measured against); byte_norms=False: the prelude's row norms from the packed float chain (what the integer dot products of the
    raw bytes are measured against); the committed stream is build().  Left unset, it follows `scaled`: the
    scaled=False baseline is the stream as it was before the scaled rotations, whole.
    rcp: 1 / c^2 of the swap-free scaled rotation from one v_rcp_f32 (rotation_scaled).  It changes the last bit of a
    scale, so it is on only in the sigma-only stream, which is not held to the bytes of its predecessor anyway; the
    stream that hands out B keeps v_rsq_f32 and the square (measured with it: profiles/r08_ab_tile_diet.log).
    sigma_only=True is the second V-free stream, csrc/wm_jacobi_sigma_gfx950.inc (written at build time), for the callers that take nothing
    but the norms (sigma_tile_dev): the columns stay scaled to the end.  No fold behind the untested sweeps; the tested
    sweeps are rotation_scaled(tested=True); every col_norms is followed by scale_norms; the scales are folded into B
    only where the 7th sweep recomputes its norms, to keep them in range up to the sweep bound (rotation_scaled)."""
    # (a shim for the tests of the scaled rotations, which hold build(scaled=False) to the instruction counts of the commit
    # before them and are not to be edited: nothing else ties the row norms to the scaling)
    byte_norms = scaled if byte_norms is None else byte_norms
    rcp = sigma_only if rcp is None else rcp
    assert scaled or not sigma_only
    st = Stream()
    e = st.emit
    Alo, Ahi = LAY.Alo, LAY.Ahi
    # inputs: %[lo0..lo7], %[hi0..hi7] raw row words; %[conv] %[skip] %[minsw] %[skipfrom]
    e(f"s_mov_b32 {SW}, 0", kind="salu")
    e(f"s_mov_b32 {EPS}, 0x{eps_literal():08x}", kind="salu")
    e(f"s_mov_b32 {CONV}, %[conv]", kind="salu")
    e(f"s_mov_b32 {SKIPC}, %[skip]", kind="salu")
    e(f"s_mov_b32 {MINSW}, %[minsw]", kind="salu")
    e(f"s_mov_b32 {SKIPFROM}, %[skipfrom]", kind="salu")
    for r in range(8):
        for c in range(8):
            src = f"%[lo{r}]" if c < 4 else f"%[hi{r}]"
            dst = Alo(r >> 1, c) if (r & 1) == 0 else Ahi(r >> 1, c)
            e(f"v_cvt_f32_ubyte{c & 3}_e32 {dst}, {src}")
    if lq:
        lq_prelude(st, byte_norms=byte_norms)
    if scaled:
        for c in range(8):
            e(f"v_mov_b32_e32 {LAY.W(c)}, 1.0")
    e(".Lwmj_lqdone_%=:", kind="label")
    st.hist.append(("nop", set()))
    e(".Lwmj_sweep_%=:", kind="label")
    e(f"s_mov_b64 {M}, 0", kind="salu")
    e(f"s_bitcmp1_b32 {SW}, 0", kind="salu")                 # norms are recomputed before odd-numbered sweeps
    e("s_cbranch_scc1 .Lwmj_nonorm_%=", kind="salu")
    if sigma_only:
        e(f"s_cmp_eq_i32 {SW}, {SIGMA_FOLD_AT}", kind="salu")
        e("s_cbranch_scc0 .Lwmj_nofold_%=", kind="salu")
        e(".Lwmj_fold_%=:", kind="label")
        fold_scales(st)
        e(".Lwmj_nofold_%=:", kind="label")
        st.hist.append(("nop", set()))
    col_norms(st)
    if scaled:
        scale_norms(st)
    e(".Lwmj_nonorm_%=:", kind="label")
    st.hist.append(("nop", set()))
    e(f"s_cmp_ge_i32 {SW}, {SKIPFROM}", kind="salu")         # pairs are skipped from sweep `skipfrom` on (0-based);
    e(f"s_cselect_b64 {NOSKIP}, 0, -1", kind="salu")         # before that every pair is rotated (zero columns must still be sorted)
    # sweeps 0 .. min_sweeps - 2 can never be the last one: they run the body without test and skip logic
    e(f"s_add_i32 {TMPS}, {SW}, 1", kind="salu")
    e(f"s_cmp_lt_i32 {TMPS}, {MINSW}", kind="salu")
    e("s_cbranch_scc0 .Lwmj_tested_%=", kind="salu")
    for p in range(7):
        for q in range(p + 1, 8):
            if scaled:
                rotation_scaled(st, p, q, f"{p}{q}", swapfree=swapfree, rcp=rcp)
            else:
                rotation(st, p, q, -1, plain=True)
    if scaled and not sigma_only:
        # behind the last untested sweep the scales are folded back into B: the tested sweeps, the final norms and the
        # pinned output registers see the true columns, as they always did
        e(f"s_add_i32 {TMPS}, {SW}, 2", kind="salu")
        e(f"s_cmp_lt_i32 {TMPS}, {MINSW}", kind="salu")
        e("s_cbranch_scc1 .Lwmj_swept_%=", kind="salu")
        e(".Lwmj_fold_%=:", kind="label")
        fold_scales(st)
    e("s_branch .Lwmj_swept_%=", kind="salu")
    e(".Lwmj_tested_%=:", kind="label")
    st.hist.append(("nop", set()))
    k = 0
    for p in range(7):
        for q in range(p + 1, 8):
            if sigma_only:
                rotation_scaled(st, p, q, f"t{p}{q}", rcp=rcp, tested=True, move_test=move_test)
            else:
                rotation(st, p, q, k, move_test=move_test)
            k += 1
    e(".Lwmj_swept_%=:", kind="label")
    st.hist.append(("nop", set()))
    e(f"s_add_i32 {SW}, {SW}, 1", kind="salu")
    e(f"s_cmp_lt_i32 {SW}, {MINSW}", kind="salu")             # the first sweeps are never the last
    e("s_cbranch_scc1 .Lwmj_sweep_%=", kind="salu")
    # A rank-deficient tile's null columns are rounding residue: their mutual cosines never fall and their TRACKED norms
    # cancel to garbage, so such a lane would hold its wave to the sweep bound and report non-convergence on a perfectly
    # good image (flat-and-gradient UI content: tests/test_gpu_parity.py::test_random_scenes_every_tile_class).  After
    # DEFI_FROM sweeps - every full-rank tile is long done - a lane with n2[7] <= 1e-10 n2[0] (the tile is flagged and
    # completed from its good columns anyway) leaves the convergence mask.
    e(f"s_cmp_lt_i32 {SW}, {DEFI_FROM}", kind="salu")
    e("s_cbranch_scc1 .Lwmj_nodef_%=", kind="salu")
    e(f"v_mul_f32_e32 {LAY.x}, 0x{struct.unpack('<I', struct.pack('<f', 1e-10))[0]:08x}, {LAY.N(0)}")
    e(f"v_mov_b32_e32 {LAY.ih}, {LAY.N(7)}")                    # (keeps the compare's operands one instruction apart)
    e(f"v_cmp_gt_f32_e32 vcc, {LAY.ih}, {LAY.x}")               # n2[7] > 1e-10 n2[0]: a full-rank tile
    e(f"s_and_b64 {M}, {M}, vcc", kind="salu")
    e(".Lwmj_nodef_%=:", kind="label")
    st.hist.append(("nop", set()))
    e(f"s_cmp_eq_u64 {M}, 0", kind="salu")
    e("s_cbranch_scc1 .Lwmj_done_%=", kind="salu")
    e(f"s_cmp_lt_i32 {SW}, {MAX_SWEEPS}", kind="salu")
    e("s_cbranch_scc1 .Lwmj_sweep_%=", kind="salu")
    e(".Lwmj_done_%=:", kind="label")
    st.hist.append(("nop", set()))
    col_norms(st)
    if sigma_only:
        scale_norms(st)
    e(f"s_mov_b64 %[more], {M}", kind="salu")
    return st


def build_v():
    """jacobi_cols_pk_v: B = A V with V accumulated from the identity, norms recomputed before every sweep, every
    pair tested and rotated; a lane (tile) whose own sweep saw nothing to rotate leaves the exec mask and sits out
    the sweeps its wave neighbours still need, so its result does not depend on which tiles share the wave."""
    L = LAY_V
    st = Stream()
    e = st.emit
    e(f"s_mov_b64 {SAVE}, exec", kind="salu")
    e(f"s_mov_b32 {SW}, 0", kind="salu")
    e(f"s_mov_b32 {EPS}, 0x{eps_literal():08x}", kind="salu")
    e(f"s_mov_b32 {CONV}, %[conv]", kind="salu")
    for rp in range(4):
        for c in range(8):
            b = L.V0 + 2 * (8 * rp + c)
            e(f"v_mov_b32_e32 v{b}, {'1.0' if 2 * rp == c else '0'}")
            e(f"v_mov_b32_e32 v{b + 1}, {'1.0' if 2 * rp + 1 == c else '0'}")
    e(".Lwmv_sweep_%=:", kind="label")
    st.hist.append(("nop", set()))
    e(f"s_mov_b64 {M}, 0", kind="salu")
    col_norms(st, L)
    for p in range(7):
        for q in range(p + 1, 8):
            rotation(st, p, q, -1, L=L, with_v=True)
    e(f"s_add_i32 {SW}, {SW}, 1", kind="salu")
    e(f"s_and_b64 exec, exec, {M}", kind="salu")              # lanes that rotated something stay (SCC = any left)
    e("s_cbranch_scc0 .Lwmv_done_%=", kind="salu")
    e(f"s_cmp_lt_i32 {SW}, {MAX_SWEEPS}", kind="salu")
    e("s_cbranch_scc1 .Lwmv_sweep_%=", kind="salu")
    e(".Lwmv_done_%=:", kind="label")
    st.hist.append(("nop", set()))
    e(f"s_mov_b64 %[more], exec", kind="salu")                # non-zero only when the sweep bound was hit
    e(f"s_mov_b32 %[sweeps], {SW}", kind="salu")
    e(f"s_mov_b64 exec, {SAVE}", kind="salu")
    col_norms(st, L)
    col_norms(st, L, of_v=True)
    return st


HEADER = """// GENERATED by tools/gen_jacobi_asm.py - do not edit.  The packed one-sided Jacobi of the tile kernels
// (raw_to_pk + jacobi_cols_pk + final col_norms2_pk of wm_tile_math.h) as one gfx950 instruction stream with
// pinned registers: B = X V in v[40:103] (a[rp][c] = v[40 + 2 (8 rp + c)] : rows 2 rp, 2 rp + 1),
// |b_c|^2 in v[104:111], temporaries v[112:127], the squared column scales of the scaled rotations in v[128:135]
// (through the untested sweeps the registers of B hold a_c / sqrt(w_c); the scales are folded back behind the last of them),
// control in s[80:98].  {n_inst} instructions, {n_nop} s_nop.
// The sweeps run on B0 = X Q, the row-pivoted Householder LQ of the tile applied from the right (its column Gram
// matrix is one QR-algorithm step further on: about one sweep fewer); B stays X * orthogonal.
//   conv2:     a sweep that saw no pair with cos^2 > conv2 in any tile of the wave, and no rotation that moved the two
//              squared norms by w with w^2 > {move2:g} n2[0] max(n2[p], n2[q]) (JAC_MOVE2), is the last one
//   skip2:     from sweep `skip_from` (0-based) on, a pair below skip2 in every tile of the wave is left alone
//   min_sweeps: sweeps that run regardless of the test (the first ones never pass it)
// Returns the wave's not-converged mask after the last sweep (non-zero only when the bound of {max_sw} is hit).
__device__ __forceinline__ unsigned long long jacobi_cols_gfx950(const uint32_t (&lo)[8], const uint32_t (&hi)[8],
                                                                 wm::v2f (&a)[4][8], float (&n2)[8], const float conv2,
                                                                 const float skip2, const int min_sweeps,
                                                                 const int skip_from) {{
  unsigned long long more;
  asm volatile(
"""

HEADER_V = """// GENERATED by tools/gen_jacobi_asm.py - do not edit.  jacobi_cols_pk_v of wm_tile_math.h (one-sided Jacobi WITH V:
// the fallback embed of rank-deficient tiles and the watermark-side SVD) as one gfx950 instruction stream with pinned
// registers: B = A V in v[40:103], V in v[104:167] (both [rp][c] -> base + 2 (8 rp + c), rows 2 rp, 2 rp + 1),
// |b_c|^2 in v[168:175], |v_c|^2 in v[176:183], temporaries v[184:199], control in s[80:89].
// {n_inst} instructions, {n_nop} s_nop.  Every pair is tested (cos^2 > conv2) and rotated; norms are recomputed
// before every sweep; a lane whose own sweep rotated nothing leaves the exec mask (restored at the end).
// Included inside namespace wm.  Returns sweeps, negated when the bound of {max_sw} was hit with lanes still active.
__device__ __forceinline__ int jacobi_cols_v_gfx950(v2f (&a)[4][8], v2f (&v)[4][8], float (&n2)[8], float (&vn2)[8],
                                                    const float conv2) {{
  unsigned long long more;
  int sweeps;
  asm volatile(
"""


def csrc_path(name):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "digital-watermarking-for-image-video-using-dct-svd-singular-value-decomposition_amd", "csrc", name)


def n_instructions(st):
    return sum(1 for ln in st.lines if not ln.endswith(":"))


def render():
    st = build()
    body = HEADER.format(n_inst=n_instructions(st), n_nop=st.nops(), max_sw=MAX_SWEEPS, move2=MOVE2)
    for ln in st.lines:
        body += f'      "{ln}\\n\\t"\n'
    outs = []
    for rp in range(4):
        for c in range(8):
            b = A0 + 2 * (8 * rp + c)
            outs.append(f'"=&{{v[{b}:{b + 1}]}}"(a[{rp}][{c}])')
    for c in range(8):
        outs.append(f'"=&{{v{N0 + c}}}"(n2[{c}])')
    outs.append('[more] "=&s"(more)')
    ins = [f'[lo{r}] "v"(lo[{r}])' for r in range(8)] + [f'[hi{r}] "v"(hi[{r}])' for r in range(8)]
    ins += ['[conv] "s"(conv2)', '[skip] "s"(skip2)', '[minsw] "s"(min_sweeps)', '[skipfrom] "s"(skip_from)']
    clob = [f'"v{i}"' for i in range(T, LAY.W0 + 8)] + [f'"s{i}"' for i in range(80, 99)] + ['"vcc"', '"scc"']
    body += "      : " + ",\n        ".join(outs) + "\n"
    body += "      : " + ",\n        ".join(ins) + "\n"
    body += "      : " + ", ".join(clob) + ");\n  return more;\n}\n"
    return st, body


HEADER_SIGMA = """// GENERATED by tools/gen_jacobi_asm.py - do not edit.  The sigma-only form of the stream in wm_jacobi_gfx950.inc
// (build(sigma_only=True)), for the kernels that take nothing but the singular values: same prelude, same sweep control,
// same tests, but the columns stay SCALED to the end - v[40:103] hold a_c / sqrt(w_c), v[128:135] the squared scales w_c,
// the tested sweeps rotate the scaled columns too and every recomputed norm is multiplied by its scale.  Nothing folds
// the scales into B except once ahead of the 7th sweep's norms (range of the scales up to the sweep bound).  B does not
// leave the stream: only |b_c|^2 in v[104:111].  {n_inst} instructions, {n_nop} s_nop.
// Returns the wave's not-converged mask after the last sweep (non-zero only when the bound of {max_sw} is hit).
__device__ __forceinline__ unsigned long long jacobi_sigma_gfx950(const uint32_t (&lo)[8], const uint32_t (&hi)[8],
                                                                  float (&n2)[8], const float conv2, const float skip2,
                                                                  const int min_sweeps, const int skip_from) {{
  unsigned long long more;
  asm volatile(
"""


def render_sigma():
    st = build(sigma_only=True)
    body = HEADER_SIGMA.format(n_inst=n_instructions(st), n_nop=st.nops(), max_sw=MAX_SWEEPS)
    for ln in st.lines:
        body += f'      "{ln}\\n\\t"\n'
    outs = [f'"=&{{v{N0 + c}}}"(n2[{c}])' for c in range(8)] + ['[more] "=&s"(more)']
    ins = [f'[lo{r}] "v"(lo[{r}])' for r in range(8)] + [f'[hi{r}] "v"(hi[{r}])' for r in range(8)]
    ins += ['[conv] "s"(conv2)', '[skip] "s"(skip2)', '[minsw] "s"(min_sweeps)', '[skipfrom] "s"(skip_from)']
    clob = [f'"v{i}"' for i in range(A0, N0)] + [f'"v{i}"' for i in range(T, LAY.W0 + 8)]
    clob += [f'"s{i}"' for i in range(80, 99)] + ['"vcc"', '"scc"']
    body += "      : " + ",\n        ".join(outs) + "\n"
    body += "      : " + ",\n        ".join(ins) + "\n"
    body += "      : " + ", ".join(clob) + ");\n  return more;\n}\n"
    return st, body


def write_sigma(out=None):
    """csrc/wm_jacobi_sigma_gfx950.inc is a build product: the package's build() calls this ahead of hipcc, `--write`
    writes it too, git ignores it.  Why it is not committed like its two siblings: it is 5 800 generated lines that differ
    from wm_jacobi_gfx950.inc only in what rotation_scaled(tested=True), the missing fold and scale_norms put there, and a
    change that carries them cannot be read.  What is committed instead is what decides its text - this generator - and
    its fingerprint: tests/test_jacobi_sigma_scaled.py holds the instruction count and the SHA-256 of the rendered file,
    so a change to the generator that changes what the sigma-only kernels run shows as a changed fingerprint in the
    diff, and `--check` compares a file that is present.  Written only where the content differs, so that an
    up-to-date library is not rebuilt."""
    out = out or csrc_path("wm_jacobi_sigma_gfx950.inc")
    body = render_sigma()[1]
    if not os.path.exists(out) or open(out).read() != body:
        open(out, "w").write(body)
    return out


def render_v():
    L = LAY_V
    st = build_v()
    body = HEADER_V.format(n_inst=n_instructions(st), n_nop=st.nops(), max_sw=MAX_SWEEPS)
    for ln in st.lines:
        body += f'      "{ln}\\n\\t"\n'
    outs = []
    for rp in range(4):
        for c in range(8):
            b = L.A0 + 2 * (8 * rp + c)
            outs.append(f'"+{{v[{b}:{b + 1}]}}"(a[{rp}][{c}])')
    for rp in range(4):
        for c in range(8):
            b = L.V0 + 2 * (8 * rp + c)
            outs.append(f'"=&{{v[{b}:{b + 1}]}}"(v[{rp}][{c}])')
    for c in range(8):
        outs.append(f'"=&{{v{L.N0 + c}}}"(n2[{c}])')
    for c in range(8):
        outs.append(f'"=&{{v{L.VN0 + c}}}"(vn2[{c}])')
    outs += ['[more] "=&s"(more)', '[sweeps] "=&s"(sweeps)']
    ins = ['[conv] "s"(conv2)']
    clob = [f'"v{i}"' for i in range(L.T, L.T + 16)] + [f'"s{i}"' for i in range(80, 90)] + ['"vcc"', '"scc"']
    body += "      : " + ",\n        ".join(outs) + "\n"
    body += "      : " + ",\n        ".join(ins) + "\n"
    body += "      : " + ", ".join(clob) + ");\n  return more ? -sweeps : sweeps;\n}\n"
    return st, body


def main():
    import argparse
    ap = argparse.ArgumentParser(description="Generate the gfx950 Jacobi instruction streams (csrc/wm_jacobi*_gfx950.inc). "
                                 "Default: compare with the committed files and write nothing.")
    ap.add_argument("--write", action="store_true", help="rewrite a file whose content differs (an identical file is "
                    "never touched: its mtime would otherwise make build() recompile libwmhip.so)")
    ap.add_argument("--check", action="store_true", help="compare only (the default); exit status 1 on a difference")
    args = ap.parse_args()
    differs = False
    for name, fn in (("wm_jacobi_gfx950.inc", render), ("wm_jacobi_sigma_gfx950.inc", render_sigma),
                     ("wm_jacobi_v_gfx950.inc", render_v)):
        st, body = fn()
        out = csrc_path(name)
        old = open(out).read() if os.path.exists(out) else None
        what = f"{os.path.normpath(out)}: {n_instructions(st)} instructions, {st.nops()} s_nop"
        if old is None and fn is render_sigma and not args.write:      # a build product: absent from a clean checkout
            print("not built   " + what + "   (written by --write and by the package's build())", file=sys.stderr)
        elif old == body:
            print("up to date  " + what, file=sys.stderr)
        elif args.write and not args.check:
            open(out, "w").write(body)
            print("wrote       " + what, file=sys.stderr)
        else:
            differs = True
            print("DIFFERS     " + what + "   (run with --write to regenerate)", file=sys.stderr)
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
