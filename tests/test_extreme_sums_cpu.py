"""The worst-case sums of every tap table, on the CPU: the closed form against the oracle, rails and peaks, and the headroom table.

tests/adversarial.py builds streams whose windows drive v = sum q s, every base-32 digit sum, every f32 part of the fp6 recombination and every
int8 limb sum to its attainable extreme.  Here, without a GPU:
  * the oracle's f64 output at every window equals exact * 2^-S with ==, for every filter that serves frames on both tap grids and for every
    composed polyphase table (a first-principles pin of the oracle: `exact` comes from filters/filter_tables.json in Python integers);
  * at 24 bits the same streams reach both rails and the peak is sum|q| 2^-S exactly;
  * the headroom table: the attainable extreme of every f32 part (the sum over the positive or over the negative entries, not sum|.|, which is
    what mx_exact / mx_wide_exact / px_exact bound) stays below 2^24, and |v| below 2^31.  DESIGN.md section 2 quotes the printed table.
tests/test_gpu_extreme_sums.py runs the same streams through every kernel route."""
import numpy as np
import pytest

import adversarial as A
from helpers import decode_pcm

FIR_CASES = [(n, g, False) for n in A.FRAME_FILTERS for g in (24, 32)] + [("E_M32", 24, True), ("D_M8", 32, True)]      # (table, tap grid, MSB first)
POLY_CASES = [(n, False) for n in sorted(A.POLYS)] + [("P_2_384000", True)]


def _fir_oracle(O, name, msb, **kw):
    dsd_rate, out_rate, filt = A.FRAME_FILTERS[name]
    return O.Oracle(dsd_rate=dsd_rate, output_rate=out_rate, channels=1, fmt="P", endianness="M" if msb else "L", block_size=4096, filter=filt, **kw)


def _poly_oracle(O, name, msb, **kw):
    dsd_rate, out_rate = A.POLYS[name]
    return O.Oracle(dsd_rate=dsd_rate, output_rate=out_rate, channels=1, fmt="P", endianness="M" if msb else "L", block_size=4096, filter="E", **kw)


def _assert_closed_form(st, y):
    idx = np.array([n for n, _, _ in st.windows])
    want = np.array([ex * 2.0 ** -st.S for _, _, ex in st.windows])            # exact in f64: |exact| < 2^40
    assert idx[-1] < y.shape[0]
    bad = np.flatnonzero(y[idx, 0] != want)
    assert bad.size == 0, [(st.windows[i][:2], y[idx[i], 0], want[i]) for i in bad[:3]]
    # the windows do what they are for: `whole` reaches +sum|q| and -sum|q| (of the worst phase of a polyphase table)
    assert max(e for _, k, e in st.windows if k == "whole+") == st.sum_abs and min(e for _, k, e in st.windows if k == "whole-") == -st.sum_abs


@pytest.mark.parametrize("name,grid,msb", FIR_CASES)
def test_oracle_equals_the_closed_form_at_every_window(oracle_mod, name, grid, msb):
    M = A.tables()["filters"][name]["M"]
    st = A.build_fir(name, tap_bits=grid, T=A.WIDE_TILE.get(M, A.FIR_TILE[M]) if grid == 32 else A.FIR_TILE[M], seed=5, msb_first=msb)
    o = _fir_oracle(oracle_mod, name, msb, bit_depth=32, dither="X", tap_bits=grid)
    info = o.info()
    assert info["S"] + (8 if grid == 32 else 0) == st.S and info["M"] == M
    _, frames, y = o.translate(st.packed(msb), want_f64=True)
    _assert_closed_form(st, y[:frames])
    assert o.peak(0) == st.sum_abs * 2.0 ** -st.S


@pytest.mark.parametrize("name,msb", POLY_CASES)
def test_oracle_equals_the_closed_form_on_the_polyphase_tables(oracle_mod, name, msb):
    st = A.build_poly(name, T=160 * A.POLY_GROUPS[name], seed=6)
    o = _poly_oracle(oracle_mod, name, msb, bit_depth=32, dither="X")
    _, frames, y = o.translate(st.packed(msb), want_f64=True)
    _assert_closed_form(st, y[:frames])
    assert o.peak(0) == st.sum_abs * 2.0 ** -st.S


@pytest.mark.parametrize("name", list(A.FRAME_FILTERS) + sorted(A.POLYS))
def test_rails_and_peak_at_24_bits(oracle_mod, name):
    """24-bit TPDF at 0 dB: an overshoot of 1.3 to 1.6 full scale clips on both sides, and the peak is the table's sum|q| 2^-S exactly"""
    if name in A.POLYS:
        st = A.build_poly(name, T=160 * A.POLY_GROUPS[name], seed=7)
        o = _poly_oracle(oracle_mod, name, False, bit_depth=24, dither="T", seed=3)
    else:
        st = A.build_fir(name, T=A.FIR_TILE[A.tables()["filters"][name]["M"]], seed=7)
        o = _fir_oracle(oracle_mod, name, False, bit_depth=24, dither="T", seed=3)
    out, frames = o.translate(st.packed())
    pcm = decode_pcm(out[:frames * 3], 24, 1)
    assert pcm.max() == (1 << 23) - 1 and pcm.min() == -(1 << 23)
    peak = st.sum_abs * 2.0 ** -st.S
    assert 1.25 < peak < 1.65 and o.peak(0) == peak


def test_streams_cover_every_kind_at_every_residue_and_stay_small():
    """the builder's own assertion, spelt out once: (kind, n mod T) is complete, windows are disjoint, the stream is under 2 MiB"""
    for st, nk in ((A.build_fir("E_M128", T=192), 24), (A.build_fir("E_M64", tap_bits=32, T=256), 22), (A.build_poly("P_4_384000", T=480), 16)):
        assert len(st.kind_names) == nk and st.nbytes < 2 << 20
        assert {(k, n % st.T) for n, k, _ in st.windows} == {(k, r) for k in st.kind_names for r in range(st.T)}
        idx = [n for n, _, _ in st.windows]
        assert all(b - a == st.W for a, b in zip(idx[:-1], idx[1:]))
    # the other channel of a pair never holds the same kind at the same time
    a, b = A.build_fir("E_M8", T=512), A.build_fir("E_M8", T=512, rot=(1, 2))
    assert all(x[1] != y[1] and x[0] == y[0] for x, y in zip(a.windows, b.windows))


def _extreme(p, start=0):
    """the attainable extreme of sum_{bits set} p_j - start over all bit patterns"""
    p = np.asarray(p, dtype=np.int64)
    return max(abs(int(p[p > 0].sum()) - start), abs(int(p[p < 0].sum()) - start))


def _headroom(g, S, M=0, wide=None):
    """fractions of 2^24 (the f32 parts) and of 2^31 (|v|): what a stream can attain, and in brackets the sum|.| bound the engine checks"""
    m128 = M == 128
    fp = A.f32_parts(g, 5, m128=m128)
    # the accumulators of the digit-4 rows start from -2^(S-20): -2^(S-15) in hi = S3 + 32 S4, -2^(S-10) in the M = 128 form's S2 + 32 S3 + 1024 S4
    # (the dithered integer depths below M = 128 start them from zero and add the -2^S later: hi is then smaller than what is computed here)
    start = 1 << (S - 10 if m128 else S - 15)
    row = {"lo": (_extreme(fp["lo"]), int(np.abs(fp["lo"]).sum())), "hi": (_extreme(fp["hi"], start), int(np.abs(fp["hi"]).sum()) + start)}
    if wide is not None:
        wp = A.f32_parts(wide, 7)
        for k in ("lo", "mid", "hi"):
            row["w" + k] = (_extreme(wp[k]), int(np.abs(wp[k]).sum()))
    row["v"] = (int(np.abs(g).sum()), int(np.abs(g).sum()))
    return row


def test_headroom_table():
    """computed, not measured: every attainable f32 part below 2^24 and |v| = sum|q| below 2^31, for every filter and every polyphase phase"""
    lines = []
    for name, t in A.tables()["filters"].items():
        g, S, M = A.fir_taps(name)
        row = _headroom(g, S, M, wide=A.fir_taps(name, 32)[0])
        lines.append((name, S, row))
    for name in sorted(A.POLYS):
        q2, t = A.poly_taps(name)
        rows = [_headroom(q2[rho], t["S"]) for rho in range(t["Lp"])]
        assert all(int(q2[rho].sum()) == 1 << t["S"] for rho in range(t["Lp"]))       # unity DC gain per phase: the start value assumes it
        lines.append((name, t["S"], {k: max(r[k] for r in rows) for k in rows[0]}))    # the worst phase
    print("\ntable        S   lo/2^24        hi/2^24        32-bit grid: lo, mid, hi /2^24              |v|/2^31  |v|/2^S")
    for name, S, row in lines:
        f = lambda k: "%.3f (%.3f)" % (row[k][0] / 2.0 ** 24, row[k][1] / 2.0 ** 24)
        wide = "  ".join(f(k) for k in ("wlo", "wmid", "whi")) if "wlo" in row else ""
        print("%-11s %2d   %s  %s  %-43s %.3f     %.3f" % (name, S, f("lo"), f("hi"), wide, row["v"][0] / 2.0 ** 31, row["v"][0] / 2.0 ** S))
        for k, (att, bound) in row.items():
            lim = 1 << 31 if k == "v" else 1 << 24
            assert att <= bound
            assert att < lim, (name, k, att)
            if not (k.startswith("w") and not _one_pass(name)):
                assert bound < lim, (name, k, bound)                                   # what mx_exact / px_exact / mx_wide_exact require
        # the int8 kernels' biased form v0 = v + 2^S = 2 sum_{bits set} q in an int32: their own condition 2^S + sum|q| < 2^31 (E_M128 takes the other form)
        if S <= 29:
            assert (1 << S) + row["v"][0] < 1 << 31


def _one_pass(name):
    """the one-pass form of the 32-bit grid exists for E_M32 and E_M64 (D2D_MX_UNIT_LIST: MX_WIDE); other tables' seven-digit bounds are not relied on"""
    return name in ("E_M32", "E_M64")
