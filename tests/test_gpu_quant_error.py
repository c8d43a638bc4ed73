"""quant_error against x^ = dequant_ref(quant_ref(page)) in numpy float64: both
codecs, four client layouts, the edges of the lane mapping; refusals; a real
write + read; quant_report. Maxima and counts are exact; every term of the two
sums is exact in float64, so two summation orders of a part's n terms differ by
at most n * 2^-52 relative: that is the bound."""

import uuid

import numpy as np
import pytest
import torch

import infinistore_amd as ifs
from infinistore_amd import _native
from infinistore_amd.kv_connector import PagedKVConnector

from _kernel_refs import bf16_bits, bf16_from_bits, fp8_dequant_ref, fp8_quant_ref
from _mxfp4_refs import roundtrip_ref
from test_gpu import gpu_server, local_conn  # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

# segment sizes: one element unit, and one lane sweep of the workgroup below,
# at and above (fp8: 512 lanes x 8 elements; mxfp4: kMxfp4GroupsPerIter groups)
SWEEP = {"fp8": 512 * 8, "mxfp4": _native._MXFP4_GROUPS_PER_ITER * 32}
UNIT = {"fp8": 8, "mxfp4": 32}
SEGS = {q: [UNIT[q], SWEEP[q] - UNIT[q], SWEEP[q], SWEEP[q] + UNIT[q]] for q in SWEEP}
# layout -> (tensors G, 0 for `cache=`; total segments S)
LAYOUTS = {"contiguous": (0, 1), "two_segments": (0, 2), "three_tensors": (3, 3),
           "two_tensors_two_segments": (2, 4)}
F = ifs.QuantErrorFields()


def _pages(nb, P, n, seed=0):
    """[nb, P, n] bf16, five kinds of page in turn: randn x logspace(-3, 3); the
    absmax in the LAST part and the first about 1000 times smaller; an all-zero
    part; NaN, +inf and -inf in the last part; plain randn."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(nb, P, n, generator=g)
    x[0::5] *= torch.logspace(-3, 3, P * n).reshape(P, n)
    x[1::5, 0] *= 1e-3
    x[1::5, -1, -1] = 30.0
    x[2::5, 0] = 0
    x[3::5, -1, :3] = torch.tensor([float("nan"), float("inf"), float("-inf")])
    return x.to(torch.bfloat16)


def _place(pages, S, G):
    """Tensor g (one for G == 0) is [S/G, nb + 1, seg] on the device, page i in
    row table[i], tensors in DESCENDING address order -> (quant_error kwargs, tensors)."""
    nb, seg = pages.shape[0], pages.numel() // (pages.shape[0] * S)
    T = max(G, 1)
    per = S // T
    table = torch.randperm(nb, generator=torch.Generator().manual_seed(nb))
    buf = torch.zeros(T, per, nb + 1, seg, dtype=torch.bfloat16)
    buf[:, :, table] = pages.reshape(nb, T, per, seg).permute(1, 2, 0, 3)
    buf = buf.flip(0).contiguous().to("cuda:0")
    tensors = [buf[T - 1 - g].reshape(-1) for g in range(T)]
    kw = dict(offsets=(table * seg).tolist(), page_size=S * seg, segments=S,
              segment_stride=(nb + 1) * seg)
    kw.update(dict(cache=None, tensors=tensors) if G else dict(cache=tensors[0]))
    return kw, tensors


def _fields(x, xh):
    """[..., n] float64 x and x^ -> [..., 5]."""
    ok = np.isfinite(x) & np.isfinite(xh)
    x, d = np.where(ok, x, 0), np.where(ok, x, 0) - np.where(ok, xh, 0)
    return np.stack([(x * x).sum(-1), (d * d).sum(-1), np.abs(d).max(-1), np.abs(x).max(-1),
                     (~ok).sum(-1).astype(np.float64)], -1)


def _reference(pages, quant):
    nb, P, n = pages.shape
    flat = pages.reshape(nb, P * n)
    xh = (fp8_dequant_ref(*fp8_quant_ref(flat)) if quant == "fp8"
          else bf16_from_bits(roundtrip_ref(flat))).double().numpy()
    return _fields(pages.double().numpy(), xh.reshape(nb, P, n))


def _assert_fields(got, ref, n, what=""):
    got = got.numpy() if isinstance(got, torch.Tensor) else got
    assert np.array_equal(got[..., 2:], ref[..., 2:]), what
    assert (np.abs(got[..., :2] - ref[..., :2]) <= ref[..., :2] * n * 2.0 ** -52).all(), what


@pytest.mark.parametrize("nb", [1, 40])
@pytest.mark.parametrize("seg_i", range(4))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("quant", ["fp8", "mxfp4"])
def test_fields_equal_reference(quant, layout, seg_i, nb):
    G, S = LAYOUTS[layout]
    P = G or S
    n = SEGS[quant][seg_i] * S // P
    pages = _pages(nb, P, n, seed=seg_i)
    ref = _reference(pages, quant)
    kw, tensors = _place(pages, S, G)
    before = [bf16_bits(t) for t in tensors]
    got = ifs.quant_error(quant=quant, **kw)
    assert got.shape == (nb, P, 5) and got.dtype == torch.float64
    _assert_fields(got, ref, n, f"{quant} {layout} n={n} nb={nb}")
    assert torch.equal(got.view(torch.int64), ifs.quant_error(quant=quant, **kw).view(torch.int64))
    assert all(np.array_equal(bf16_bits(t), b) for t, b in zip(tensors, before))
    if nb == 40:  # the special pages said what they were built to say
        assert (ref[2::5, 0, :4] == 0).all() and (got[2::5, 0, :4] == 0).all()
        bad = 32 if quant == "mxfp4" else 3  # a NaN takes its whole group of 32 along
        assert (got[3::5, -1, F.nonfinite] == bad).all()
    if nb == 40 and quant == "fp8" and S == P > 1:
        # the quiet first part of the pages whose last part is loud: its relative
        # error exceeds that of the same data probed alone, by the reference's factor
        alone = ifs.quant_error(tensors[0], kw["offsets"][1::5], n, "fp8")[:, 0].numpy()
        ref_alone = _reference(pages[1::5, :1], "fp8")[:, 0]
        _assert_fields(alone, ref_alone, n, "alone")
        rel = [e[:, F.sum_sq_err] / e[:, F.sum_sq]
               for e in (got[1::5, 0].numpy(), alone, ref[1::5, 0], ref_alone)]
        assert (rel[2] > rel[3]).all() and (rel[0] > rel[1]).all()
        assert np.allclose(rel[0] / rel[1], rel[2] / rel[3], rtol=4 * n * 2.0 ** -52, atol=0)


SENTINEL = -12345.0
REFUSED = {  # kwargs of _native.quant_error on top of a legal request
    "no_codec": dict(codec_flag=0), "misaligned_base": dict(base_add=2),
    "misaligned_stride": dict(n_segments=2, segment_stride=64 * 2 + 2),
    "17_elements": dict(elems_per_block=17), "129_tensors": dict(n_tensors=129),
    "segments_do_not_divide": dict(elems_per_block=64, n_segments=3, segment_stride=256)}


@pytest.mark.parametrize("case", REFUSED)
@pytest.mark.parametrize("flag", [m[0] for m in ifs.InfinityConnection.QUANT_MODES.values()])
def test_launcher_refusals_leave_the_output_untouched(flag, case):
    kw = dict(REFUSED[case])
    src = torch.zeros(4096, dtype=torch.bfloat16, device="cuda:0")
    out = torch.full((129 * 5,), SENTINEL, dtype=torch.float64).pin_memory()
    bases = [src.data_ptr()] * kw.pop("n_tensors", 0)
    base = 0 if bases else src.data_ptr() + kw.pop("base_add", 0)
    args = dict(elems_per_block=128, codec_flag=flag, n_segments=max(len(bases), 1))
    args.update(kw)
    with pytest.raises(ValueError):
        _native.quant_error(base, [0], device=0, bases=bases, out_ptr=out.data_ptr(), **args)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


@pytest.mark.parametrize("G", [0, 2])
@pytest.mark.parametrize("quant", ["fp8", "mxfp4"])
def test_probe_equals_a_real_write_and_read(gpu_server, quant, G):
    """The fields of the source against what the server returns for it."""
    nb, S = 5, max(G, 1)
    n = SWEEP[quant] + UNIT[quant]
    pages = _pages(nb, S, n, seed=3)
    kw, tensors = _place(pages, S, G)
    outs = [torch.full_like(t, 7.0) for t in tensors]
    keys = [f"qerr-{uuid.uuid4().hex[:12]}-{i}" for i in range(nb)]
    conn = local_conn(gpu_server)
    try:
        if G:
            ts, ts2 = conn.register_tensor_set(tensors), conn.register_tensor_set(outs)
            conn.write_pages(None, keys, kw["offsets"], S * n, sync=True, quant=quant,
                             tensor_set=ts)
            conn.read_pages(None, keys, kw["offsets"], S * n, tensor_set=ts2)
        else:
            conn.write_pages(tensors[0], keys, kw["offsets"], n, sync=True, quant=quant)
            conn.read_pages(outs[0], keys, kw["offsets"], n)
        conn.sync()
        rows = torch.tensor(kw["offsets"]) // n
        x, xh = (torch.stack([t.reshape(nb + 1, n)[rows] for t in ts_], 1).double().cpu().numpy()
                 for ts_ in (tensors, outs))
        _assert_fields(ifs.quant_error(quant=quant, **kw), _fields(x, xh), n, f"{quant} G={G}")
    finally:
        conn.delete_keys(keys)
        conn.close()


def test_quant_report_fused_fp8_costs_the_quiet_layer(gpu_server):
    n, nb = 512, 4
    g = torch.Generator().manual_seed(1)
    quiet = (torch.randn(nb * n, generator=g) * 1e-2).to(torch.bfloat16)
    loud = (torch.randn(nb * n, generator=g) * 10).to(torch.bfloat16)
    layers = [quiet.to("cuda:0"), loud.to("cuda:0")]
    offs = [i * n for i in range(nb)]
    kvc = PagedKVConnector("127.0.0.1", gpu_server, "qerr", n_layers=2)
    try:
        fused = kvc.quant_report(layers, offs, "fp8", n)
        single = kvc.quant_report(layers[0], offs, "fp8", n)
    finally:
        kvc.close()
    ref = _reference(torch.stack([quiet.reshape(nb, n), loud.reshape(nb, n)], 1), "fp8").sum(0)
    want = 10 * np.log10(ref[:, F.sum_sq] / ref[:, F.sum_sq_err])
    assert np.allclose([r["snr_db"] for r in fused], want, rtol=1e-12, atol=0)
    assert [r["absmax"] for r in fused] == [float(quiet.abs().max()), float(loud.abs().max())]
    assert fused[0]["snr_db"] < single[0]["snr_db"] and fused[0]["nonfinite"] == 0
