"""The pipelined int8 FIR kernel is compiled from one list: D2D_M3_UNIT_LIST (dsd2dxd_amd/csrc/d2d_m3.h), one object per row."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_filter_has_a_compiled_shape():
    """every row of D2D_FILTERS (filters/filter_tables.inc) with M <= 64 meets a row of D2D_M3_UNIT_LIST with its (MB, NPG), and every filter
    that serves frames (all but the cascade's stage-A filters) one that names its tap count: a regenerated table whose length moved would
    otherwise fall to the slower int8 kernels without a word"""
    with open(os.path.join(ROOT, "filters", "filter_tables.inc")) as f:
        inc = f.read()
    body = re.search(r"D2D_FILTERS\[(\d+)\] = \{(.*?)\n\};", inc, re.S)
    filters = [(n, int(m), int(t)) for n, m, t in re.findall(r'\{ "(\w+)", \'\w\', (\d+), (\d+),', body.group(2))]
    assert len(filters) == int(body.group(1))
    with open(os.path.join(ROOT, "dsd2dxd_amd", "csrc", "d2d_m3.h")) as f:
        hdr = f.read()
    lst = re.search(r"#define D2D_M3_UNIT_LIST\(X\)(.*?)\n[^ ]", hdr, re.S).group(1)
    rows = [tuple(int(x) for x in r) for r in re.findall(r"X\((\d+), (\d+), (\d+), (\d+), (\d+)\)", lst)]
    assert len(rows) == lst.count("X(")
    scratch = {r[1:3] for r in rows}                                   # every row holds the scratch flavour
    frames = {(r[1], r[2], nt) for r in rows for nt in r[3:] if nt}
    served = [f for f in filters if f[1] <= 64]
    assert len(served) == 15
    for name, M, N in served:
        MB, NPG = M // 8, (N + 7 * M + 24 + 63) // 64
        assert (MB, NPG) in scratch, f"{name}: no compiled d2d_fir_mfma3_kernel writes the scratch for (MB, NPG) = ({MB}, {NPG})"
        if not name.startswith("A_"):
            assert (MB, NPG, N) in frames, f"{name}: no compiled d2d_fir_mfma3_kernel serves frames for (MB, NPG, taps) = ({MB}, {NPG}, {N})"
    units = [r[0] for r in rows]
    assert units == list(range(len(rows))), f"D2D_M3_UNIT_LIST: the units are not numbered 0 .. n-1 as the build numbers them: {units}"
    with open(os.path.join(ROOT, "dsd2dxd_amd", "csrc", "Makefile")) as f:
        m3_units = int(re.search(r"^M3_UNITS = (\d+)$", f.read(), re.M).group(1))
    assert m3_units == len(rows), f"the Makefile's M3_UNITS = {m3_units}, D2D_M3_UNIT_LIST has {len(rows)} rows"
