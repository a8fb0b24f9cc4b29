"""The device image of every net kind (csrc/dpi_net_image.h) against a numpy restatement of its
layout, on the host: a stand-alone program compiled with hipcc from the header builds the image from
a parameter file, binds the descriptor to the host blob and writes every region and scalar read
through it (tests/net_image_host.hip).  No GPU.

Restated here, independently of the header: the dense fp32 image
`W1x | w1t | b1 | c1 | W1xT | (W, WT, b) per hidden layer | wout`, zero-padded to the row stride; the
width classes and the two nx paddings (with the 96 -> 128 rule); which images a shape gets; the head's
last Linear; the fp16-split fragment order (row r, chunk u, lane group q: 8 hi halves, then 8 lo
halves of columns 32u + 4q + (j & 3) + 16(j >> 2), lo = fp16((x - hi) 2048)) and its x3 form
(prescaled by a power of two into [0.5, 1), lo unscaled).  The PISGradNet split regions and the
values of the calibrated operand scales are pinned by the GPU parity tests."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
F32, F64, U32 = np.float32, np.float64, np.uint32
ELU, TANH = 1, 2                  # DPI_ACT_*
VALUE, VALUE_GRADIENT, GRADIENT = 0, 1, 2  # DPI_HEAD_*
FO_SHAPES = {(128, 4), (128, 3), (128, 2), (64, 3), (64, 2), (32, 2), (16, 1), (16, 2), (16, 3)}
PIS_CH = 64

# (id, nx, widths, act, head, term, T)
MLP_CASES = [
    ("spec16_elu", 7, [16], ELU, VALUE, 0, 0.0),
    ("pad16_tanh", 7, [10, 10], TANH, VALUE, 0, 0.0),
    ("split32", 7, [32, 32], ELU, VALUE, 0, 0.0),
    ("both_32x3", 7, [32, 32, 32], ELU, VALUE, 0, 0.0),
    ("unequal_h64", 7, [48, 20, 33], ELU, VALUE, 0, 0.0),
    ("flagship", 100, [128] * 4, ELU, VALUE, 0, 0.0),
    ("nx70_96to128", 70, [64, 64], ELU, VALUE, 0, 0.0),
    ("nx200_224to256", 200, [32, 32], ELU, VALUE, 0, 0.0),
    ("gen_l8", 7, [24] * 8, ELU, VALUE, 0, 0.0),
    ("hc256_200_17", 7, [200, 17], ELU, VALUE, 0, 0.0),
    ("hc256_129", 7, [129], ELU, VALUE, 0, 0.0),
    ("head_vg", 7, [16], ELU, VALUE_GRADIENT, 0, 0.0),
    ("head_og_hc256", 33, [40, 130], ELU, GRADIENT, 0, 0.0),
    ("term_value", 7, [16], ELU, VALUE, 1, 0.75),
    ("term_og", 7, [16], ELU, GRADIENT, 1, 0.75),
]
PIS_CASES = [("pis_nx4_8", 4, [8], 1.0), ("pis_nx7_32x2", 7, [32, 32], 0.5)]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    if not Path(HIPCC).exists():
        pytest.fail(f"hipcc not found ({HIPCC})")
    exe = tmp_path_factory.mktemp("net_image_host") / "net_image_host"
    subprocess.run([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-o", str(exe),
                    str(ROOT / "tests" / "net_image_host.hip")], check=True)
    return exe


def run(prog, tmp_path, params, args):
    """The program's records as {name: array}."""
    pfile, ofile = tmp_path / "params.f32", tmp_path / "image.bin"
    params.tofile(pfile)
    subprocess.run([str(prog), str(ofile), str(pfile), *map(str, args)], check=True)
    out, data, pos = {}, ofile.read_bytes(), 0
    while pos < len(data):
        end = data.index(b"\n", pos)
        name, typ, cnt = data[pos:end].decode().split()
        pos = end + 1 + 4 * int(cnt)
        out[name] = np.frombuffer(data[end + 1:pos], dtype={"f32": F32, "i32": np.int32, "u32": U32}[typ])
    return out


def same_bits(got, want):
    want = np.ascontiguousarray(want).ravel()
    return got.shape == want.shape and np.array_equal(got.view(U32), want.view(U32))


def draw(seed, count):
    return (np.random.default_rng(seed).standard_normal(count) * 0.3).astype(F32)


def take_linears(params, shapes):
    """[(W (rows, cols), b (rows))] in state-dict order, and the words consumed."""
    out, pos = [], 0
    for rows, cols in shapes:
        W = params[pos:pos + rows * cols].reshape(rows, cols)
        pos += rows * cols
        out.append((W, params[pos:pos + rows]))
        pos += rows
    return out, pos


def seq_sum(a, axis):
    """The fp32 cast of the sequential fp64 sum along `axis` (np.cumsum adds in order)."""
    return np.cumsum(a.astype(F64), axis=axis).take(-1, axis=axis).astype(F32)


def dense_image(hidden, wout, nx, S, nxp, nxpT):
    (W1, b1), L = hidden[0], len(hidden)
    r0 = W1.shape[0]
    img = {k: np.zeros(S, F32) for k in ("w1t", "b1", "c1", "wout")}
    img["W1x"], img["W1xT"] = np.zeros((S, nxp), F32), np.zeros((nxpT, S), F32)
    img["W1x"][:r0, :nx] = W1[:, 1:]
    img["W1xT"][:nx, :r0] = W1[:, 1:].T
    img["w1t"][:r0], img["b1"][:r0], img["c1"][:r0] = W1[:, 0], b1, seq_sum(W1[:, 1:], 1)
    for l in range(1, L):
        W, b = hidden[l]
        full = np.zeros((S, S), F32)
        full[:W.shape[0], :W.shape[1]] = W
        img[f"W[{l}]"], img[f"WT[{l}]"] = full, full.T
        img[f"b[{l}]"] = np.zeros(S, F32)
        img[f"b[{l}]"][:len(b)] = b
    if wout is not None:
        img["wout"][:len(wout)] = wout
    return img


def frag_cols(C):
    return np.array([[32 * u + 4 * q + (j & 3) + 16 * (j >> 2) for j in range(8)]
                     for u in range(C // 32) for q in range(4)])


def pack_split(M, lo_scale=2048.0, pre_scale=1.0):
    x = (M * F32(pre_scale))[:, frag_cols(M.shape[1])]  # (R, C / 8, 8)
    with np.errstate(over="ignore"):
        hi = x.astype(np.float16)
        lo = ((x - hi.astype(F32)) * F32(lo_scale)).astype(np.float16)
    return np.concatenate([hi, lo], axis=2).ravel().view(U32)


def pack_split_x3(M):
    """(words, 2^e): M prescaled by 2^-e, max |M| = f 2^e with f in [0.5, 1); lo unscaled."""
    mx = float(np.abs(M).max())
    e = int(np.frexp(mx)[1]) if mx > 0 else 0
    return pack_split(M, 1.0, np.ldexp(1.0, -e)), F32(np.ldexp(1.0, e))


def is_pow2(x):
    m, _ = np.frexp(np.asarray(x, F64))
    return bool(np.all(np.isfinite(x)) and np.all(m == 0.5))


def check_dense(got, pre, want, L):
    names = ["W1x", "w1t", "b1", "c1", "W1xT", "wout"] + [f"{k}[{l}]" for l in range(1, L) for k in ("W", "WT", "b")]
    for k in names:
        assert same_bits(got[pre + k], want[k]), f"{pre}{k}"


@pytest.mark.parametrize("case", MLP_CASES, ids=[c[0] for c in MLP_CASES])
def test_mlp_image(prog, tmp_path, case):
    _, nx, widths, act, head, term, T = case
    n_in, L, wl, wmax = 1 + nx, len(widths), widths[-1], max(widths)
    n_out = {VALUE: 1, VALUE_GRADIENT: 1 + nx, GRADIENT: nx}[head]
    shapes = [(w, widths[l - 1] if l else n_in) for l, w in enumerate(widths)] + [(n_out, wl)]
    params = draw(len(widths) * 1000 + nx, sum(r * (c + 1) for r, c in shapes))
    linears, used = take_linears(params, shapes)
    assert used == len(params)
    hidden, (Wo, bo) = linears[:-1], linears[-1]
    got = run(prog, tmp_path, params, ["mlp", n_in, act, head, term, T, *widths])

    H = next(h for h in (16, 32, 64, 128, 256) if wmax <= h)
    HC = 128 if H <= 128 else 256
    nxg, nxg32 = -(-nx // 16) * 16, -(-nx // 32) * 32
    nxp, nxp32 = nxg, nxg32
    if nxp32 % 128 == 96:
        nxp = nxp32 = nxp32 + 32
    spec = head == VALUE and not term and L <= 4 and wmax <= 128
    gen = not spec or (H, L) not in FO_SHAPES
    scalars = {"kind": 1, "n_in": n_in, "spec": spec, "gen": gen, "head": head, "term": term, "L": L, "act": act,
               "H": HC if head else H, "nxp": nxg if head else nxp}
    for k, v in scalars.items():
        assert got[k][0] == v, k
    assert same_bits(got["term_T"], F32(T if term else 0.0))

    if spec:
        assert [got[k][0] for k in ("nxp32", "d.H", "d.L", "d.nxp", "d.act")] == [nxp32, H, L, nxp, act]
        want = dense_image(hidden, Wo[0], nx, H, nxp, nxp)
        check_dense(got, "d.", want, L)
        assert same_bits(got["d.bout"], bo[:1])
        if H % 32 == 0:
            W1x32 = np.zeros((H, nxp32), F32)
            W1x32[:, :nx] = want["W1x"][:, :nx]
            assert same_bits(got["d.W1xS"], pack_split(W1x32))
            assert same_bits(got["d.W1xTS"], pack_split(np.ascontiguousarray(W1x32.T)))
            wus = got["d.wus"]
            for l in range(1, L):
                assert same_bits(got[f"d.WS[{l}]"], pack_split(want[f"W[{l}]"])), l
                assert same_bits(got[f"d.WTS[{l}]"], pack_split(np.ascontiguousarray(want[f"WT[{l}]"]))), l
                words, scale = pack_split_x3(want[f"W[{l}]"])
                assert same_bits(got[f"d.WU[{l}]"], words), l
                assert wus[l] == scale, l
            # the operand scales: hsa[l] = 2^ea[l], hsc[l] = wus[l] / hsa[l - 1]; with Eb[l] = 2^eb[l],
            # hzs[0] = 1, hbs[0] = Eb[0], hzs[l] = wus[l] / Eb[l - 1], hbs[l] = hzs[l] Eb[l]
            hsa, hsc, hzs, hbs = (got[f"d.{k}"] for k in ("hsa", "hsc", "hzs", "hbs"))
            assert is_pow2(hsa[:L]) and is_pow2(hzs[:L]) and is_pow2(hbs[:L]) and is_pow2(hsc[1:L])
            assert hzs[0] == 1.0
            Eb = [F64(hbs[0])] + [F64(hbs[l]) / F64(hzs[l]) for l in range(1, L)]
            for l in range(1, L):
                assert F64(hsc[l]) * F64(hsa[l - 1]) == F64(wus[l]), l
                assert F64(hzs[l]) * Eb[l - 1] == F64(wus[l]), l
        else:
            for k in ("d.W1xS", "d.W1xTS"):
                assert got[k].size == 0, k
            for k in ("wus", "hsa", "hsc", "hzs", "hbs"):
                assert not got[f"d.{k}"].any(), k
    else:
        assert not any(k.startswith("d.") for k in got)

    if gen and not head:
        assert [got[k][0] for k in ("g.H", "g.L", "g.nxp", "g.act", "g.ht")] == [HC, L, nxg, act, -(-wmax // 32) * 2]
        check_dense(got, "g.", dense_image(hidden, Wo[0], nx, HC, nxg, nxg32), L)
        assert same_bits(got["g.bout"], bo[:1])
    if head:
        value = head == VALUE_GRADIENT
        assert [got[k][0] for k in ("hd.H", "hd.L", "hd.nxp", "hd.act", "hd.ht", "hd.value")] == \
            [HC, L, nxg, act, -(-wmax // 32) * 2, int(value)]
        G, bg = Wo[1:] if value else Wo, bo[1:] if value else bo
        want = dense_image(hidden, Wo[0] if value else None, nx, HC, nxg, nxg32)
        want["c1"] = np.zeros(HC, F32)
        want["c1"][:wl] = seq_sum(G, 0)  # cg[h] = sum_d G[d][h]
        wantG, wantbg = np.zeros((nxg32, HC), F32), np.zeros(nxg32, F32)
        wantG[:nx, :wl], wantbg[:nx] = G, bg
        for pre in ("hd.", "g."):  # g: the head's NetGen part
            check_dense(got, pre, want, L)
            assert same_bits(got[pre + "bout"], bo[:1] if value else F32(0.0)), pre
        assert same_bits(got["hd.G"], wantG) and same_bits(got["hd.bg"], wantbg)
        assert same_bits(got["hd.bgsum"], seq_sum(bg, 0))
    if not gen:
        assert not any(k.startswith("g.") for k in got)
    if not head:
        assert not any(k.startswith("hd.") for k in got)


@pytest.mark.parametrize("case", PIS_CASES, ids=[c[0] for c in PIS_CASES])
def test_pisgrad_image(prog, tmp_path, case):
    _, nx, hidden, T = case
    C, L = PIS_CH, len(hidden)
    nn_shapes = [(h, hidden[l - 1] if l else C + nx) for l, h in enumerate(hidden)] + [(nx, hidden[-1])]
    shapes = [(C, 2 * C), (C, C), (C, 2 * C)] + [(C, C)] * L + [(nx, C)] + nn_shapes
    params = draw(7000 + nx, 2 * C + sum(r * (c + 1) for r, c in shapes))
    phase, coeff = params[:C], params[C:2 * C]
    linears, used = take_linears(params[2 * C:], shapes)
    assert used == len(params) - 2 * C
    (te0, te0b), (te2, te2b), (sn0, sn0b) = linears[:3]
    sn, (snl, snlb), nn = linears[3:3 + L], linears[3 + L], linears[4 + L:]
    got = run(prog, tmp_path, params, ["pisgrad", nx, T, *hidden])

    for k, v in {"kind": 2, "n_in": 1 + nx, "nx": nx, "L": L, "nsm": L}.items():
        assert got[k][0] == v, k
    assert list(got["h"]) == hidden + [0] * (4 - L)
    assert same_bits(got["T"], F32(T))
    want = {"phase": phase, "coeff": coeff, "te0": te0, "te0b": te0b, "te2": te2, "te2b": te2b, "sn0": sn0,
            "sn0b": sn0b, "snlast": snl[0], "snlastb": snlb[:1]}
    for j, (W, b) in enumerate(sn):
        want[f"sn[{j}]"], want[f"snb[{j}]"] = W, b
    for l, (W, b) in enumerate(nn):
        want[f"nn[{l}]"], want[f"nnb[{l}]"] = W, b
        want[f"nnT[{l}]"] = np.ascontiguousarray((W[:, C:] if l == 0 else W).T)
        want[f"nnbP[{l}]"] = np.zeros(-(-len(b) // 64) * 64, F32)
        want[f"nnbP[{l}]"][:len(b)] = b
    for k, v in want.items():
        assert same_bits(got[k], v), k

    # smooth0 = smooth_net(emb(0))[0] in fp64: within one fp32 ulp (libm differences of a few fp64
    # ulps cannot move the fp32 cast further)
    def elu(z):
        return np.where(z > 0, z, np.expm1(z))
    d = lambda a: a.astype(F64)  # noqa: E731
    h = d(sn0) @ np.concatenate([np.sin(d(phase)), np.cos(d(phase))]) + d(sn0b)
    for W, b in sn:
        h = d(W) @ elu(h) + d(b)
    s0 = F32(d(snl[0]) @ elu(h) + d(snlb[0]))
    assert abs(F64(got["smooth0"][0]) - F64(s0)) <= F64(np.spacing(np.abs(s0)))
