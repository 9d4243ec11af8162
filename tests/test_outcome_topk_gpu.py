"""The streaming per-pair top-k over outcomes on the GPU (mdg_outcome_topk_update through ops.outcome_topk) against the dense CPU
reference (outcome_topk_ref): every comparison is torch.equal on vals and idx.  Shapes, layouts and dtypes; Lc around k and past
the prefetch depth; ties decided by the outcome id; independence of chunking and call order; skipped planes; shift / scale as two
fp32 steps; NaN and infinities; largest=False; eligible="lower"; bounded writes; refusals; and the pipeline products built on it
(highest_outcomes_of, highest_outcomes, ensemble_highest_outcomes)."""
import numpy as np
import pytest
import torch

from outcome_topk_ref import INF, outcome_topk_ref, same_state

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (33, 5), (7, 63), (5, 64), (3, 65), (33, 257)]      # one-column rows, sub-vector tails, a wave's span, a ragged last block
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
MARK_V, MARK_I = -12345.0, -7


@pytest.fixture(scope="module")
def ops():
    from madrigal_amd import ops as _ops
    return _ops


def _values(L, nh, nt, dtype, seed, kind="randn"):
    """CPU [L, nh, nt] of ``dtype``: gaussian, or drawn from {0, 1, 2, 3} (ties everywhere), or rank-like r / 16."""
    g = torch.Generator().manual_seed(seed)
    if kind == "randn":
        v = torch.randn((L, nh, nt), generator=g)
    elif kind == "small":
        v = torch.randint(0, 4, (L, nh, nt), generator=g).float()
    else:
        v = torch.randint(1, 17, (L, nh, nt), generator=g).float() / 16
    return v.to(dtype)


def _place(ops, v, layout):
    """The CPU tensor on the GPU: "pitched" (empty_scores), "contig", or "off1" -- columns 1.. of a contiguous tensor one column
    wider, whose base is aligned to the element size only."""
    L, nh, nt = v.shape
    if layout == "pitched":
        x = ops.empty_scores(L, nh, nt, "cuda", dtype=v.dtype)
    elif layout == "contig":
        x = torch.empty((L, nh, nt), dtype=v.dtype, device="cuda")
    else:
        x = torch.empty((L, nh, nt + 1), dtype=v.dtype, device="cuda")[:, :, 1:]
    x.copy_(v)
    return x


def _check(ops, x, v, k, what, **kw):
    got = ops.outcome_topk(x, k, **kw)
    assert got[0].shape == (k,) + tuple(x.shape[1:]) and got[0].dtype == torch.float32 and got[1].dtype == torch.int32
    assert got[0].stride(1) % 32 == 0 and got[0].stride() == got[1].stride()
    ref = outcome_topk_ref(v, k, **{n: (t.cpu() if isinstance(t, torch.Tensor) else t) for n, t in kw.items()})
    assert same_state(got, ref), (what, int((got[0].cpu() != ref[0]).sum()), int((got[1].cpu() != ref[1]).sum()))
    return got


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("nh,nt", SHAPES)
def test_shapes_layouts_and_dtypes(ops, nh, nt, dtype):
    """Row-pitched (16-byte lane accesses), contiguous (odd Nt: the element path) and, in 16 bits, a 2-byte-aligned base; one call
    and the same outcomes in two calls."""
    L, k = 9, 5
    v = _values(L, nh, nt, DTYPES[dtype], 10 * nh + nt)
    for layout in ("pitched", "contig", "off1"):
        x = _place(ops, v, layout)
        whole = _check(ops, x, v, k, (dtype, layout))
        st = ops.outcome_topk(x[:4], k)
        st2 = ops.outcome_topk(x[4:], k, label_base=4, state=st)
        assert st2[0] is st[0] and st2[1] is st[1]                                # updated in place
        assert torch.equal(st[0], whole[0]) and torch.equal(st[1], whole[1]), (dtype, layout, "two calls")


@pytest.mark.parametrize("k", range(1, 9))
def test_every_k_with_lc_around_k_and_past_the_prefetch_depth(ops, k):
    nh, nt = 3, 65
    for Lc in sorted({1, k - 1, k, k + 1, 67} - {0}):
        for dtype in (torch.float32, torch.bfloat16):
            v = _values(Lc, nh, nt, dtype, 100 * k + Lc)
            got = _check(ops, _place(ops, v, "pitched"), v, k, (k, Lc, dtype))
            if Lc < k:
                assert bool((got[1][Lc:] == -1).all()) and bool((got[0][Lc:] == -INF).all())          # sentinel slots
            _check(ops, _place(ops, v, "contig"), v, k, (k, Lc, dtype, "contig"))


@pytest.mark.parametrize("kind", ["small", "ranks", "copied"])
def test_ties_are_decided_by_the_outcome_id(ops, kind):
    L, nh, nt = 21, 7, 63
    v = _values(L, nh, nt, torch.float32, 7, "randn" if kind == "copied" else kind)
    labels = None
    if kind == "copied":
        v[13] = v[2]                                                             # one plane under two labels
        labels = torch.arange(L).flip(0).contiguous()                            # and the planes in descending id order
    for k in (1, 5, 8):
        for layout in ("pitched", "contig"):
            kw = {} if labels is None else {"labels": labels.cuda()}
            got = _check(ops, _place(ops, v, layout), v, k, (kind, k, layout), **kw)
            if kind == "small" and k > 1:
                same = got[0][1:] == got[0][:-1]
                assert int(same.sum()) > same.numel() // 2 and bool((got[1][1:][same] > got[1][:-1][same]).all())
            if kind == "copied" and k == 1:
                assert bool((got[1] == 7).any()) and not bool((got[1] == 18).any())          # planes 13 and 2: the lower id wins


def test_chunks_and_call_order_do_not_matter(ops):
    """L = 37: one call == chunks (5, 1, 31) folded in three shuffled orders with labels == unordered labels inside a chunk ==
    outcome_topk_merge of two half states."""
    L, nh, nt, k = 37, 33, 65, 5
    v = _values(L, nh, nt, torch.float32, 3, "ranks")
    x = _place(ops, v, "pitched")
    whole = _check(ops, x, v, k, "whole")
    ids = torch.arange(L, dtype=torch.int32, device="cuda")
    chunks = [(0, 5), (5, 6), (6, 37)]
    for order in ((2, 0, 1), (1, 2, 0), (2, 1, 0)):
        st = None
        for c in order:
            s, e = chunks[c]
            st = ops.outcome_topk(x[s:e], k, labels=ids[s:e], state=st)
        assert torch.equal(st[0], whole[0]) and torch.equal(st[1], whole[1]), order
    perm = torch.randperm(L, generator=torch.Generator().manual_seed(1))
    xs = _place(ops, v[perm], "pitched")
    got = ops.outcome_topk(xs, k, labels=perm.cuda())                            # int64 labels are converted
    assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1])
    a = ops.outcome_topk(x[:18], k)
    b = ops.outcome_topk(x[18:], k, label_base=18)
    m = ops.outcome_topk_merge(a, b)
    assert torch.equal(m[0], whole[0]) and torch.equal(m[1], whole[1])
    m = ops.outcome_topk_merge((b[0].cpu(), b[1].cpu()), (a[0].cpu(), a[1].cpu()))          # any device, either order
    assert same_state(whole, m)


def test_planes_with_a_negative_label_are_skipped(ops):
    L, nh, nt, k = 12, 5, 64, 5
    v = _values(L, nh, nt, torch.float16, 4)
    labels = torch.arange(L, dtype=torch.int32)
    labels[[0, 5, 6, 11]] = -1
    got = _check(ops, _place(ops, v, "pitched"), v, k, "skipped", labels=labels.cuda())
    keep = labels >= 0
    ref = outcome_topk_ref(v[keep], k, labels=labels[keep])                      # the same as deleting those planes
    assert same_state(got, ref)
    none = ops.outcome_topk(_place(ops, v, "pitched"), k, labels=torch.full((L,), -1, dtype=torch.int32, device="cuda"))
    assert bool((none[0] == -INF).all()) and bool((none[1] == -1).all())


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_shift_and_scale_are_a_subtract_then_a_multiply(ops, dtype):
    """Random shifts and scales: the result is bit-equal to torch's (x - shift) * scale in fp32 followed by the reference; a
    contracted FMA would differ in many entries."""
    L, nh, nt, k = 13, 33, 65, 5
    v = _values(L, nh, nt, DTYPES[dtype], 5)
    g = torch.Generator().manual_seed(6)
    shift, scale = torch.randn(L, generator=g), torch.rand(L, generator=g) + 0.25
    x = _place(ops, v, "pitched")
    for largest in (True, False):
        got = _check(ops, x, v, k, (dtype, largest), shift=shift.cuda(), scale=scale.cuda(), largest=largest)
        u = (v.float() - shift[:, None, None]) * scale[:, None, None]
        assert same_state(got, outcome_topk_ref(u, k, largest=largest))
        fused = torch.addcmul(-(shift * scale)[:, None, None].double(), v.double(), scale[:, None, None].double()).float()
        assert int((fused != u).sum()) > 0                                       # the test can tell the two apart
        _check(ops, x, v, k, (dtype, largest, "shift"), shift=shift.cuda(), largest=largest)
        _check(ops, _place(ops, v, "contig"), v, k, (dtype, largest, "scale"), scale=scale.cuda(), largest=largest)


@pytest.mark.parametrize("largest", [True, False])
def test_nan_and_infinities(ops, largest):
    L, nh, nt, k = 9, 7, 63, 5
    v = _values(L, nh, nt, torch.float32, 8)
    v[:, 0, 0] = float("nan")                                                     # a pair whose every value is NaN
    v[::2, 1, 1] = float("nan")
    v[1, 2, :] = INF
    v[3, 2, :] = INF
    v[2, 3, :] = -INF
    v[:, 4, 5] = -INF
    v[:, 4, 6] = INF
    v[:7, 5, 7] = float("nan")                                                    # two values left: sentinel slots
    for layout in ("pitched", "contig"):
        got = _check(ops, _place(ops, v, layout), v, k, (largest, layout), largest=largest)
        sent = -INF if largest else INF
        assert bool((got[0][:, 0, 0] == sent).all()) and bool((got[1][:, 0, 0] == -1).all())
        assert bool((got[1][2:, 5, 7] == -1).all()) and bool((got[1][:2, 5, 7] >= 7).all())
        assert not bool(torch.isnan(got[0]).any())
    v16 = v.to(torch.bfloat16)
    _check(ops, _place(ops, v16, "pitched"), v16, k, (largest, "bf16"), largest=largest)


@pytest.mark.parametrize("N", [33, 257])
def test_eligible_lower(ops, N):
    """A fresh state: entries with i <= j hold the sentinels; an update of a state prefilled with a marker leaves them untouched."""
    L, k = 7, 5
    v = _values(L, N, N, torch.float32, N)
    upper = (torch.arange(N)[None, :] >= torch.arange(N)[:, None]).cuda()
    for layout in ("pitched", "contig"):
        x = _place(ops, v, layout)
        got = _check(ops, x, v, k, ("lower", layout), eligible="lower")
        assert bool((got[0][:, upper] == -INF).all()) and bool((got[1][:, upper] == -1).all())
        vals = torch.full((k, N, N + (3 if layout == "contig" else 7)), MARK_V, device="cuda")[:, :, :N]
        idx = torch.full(vals.shape[:2] + (vals.stride(1),), MARK_I, dtype=torch.int32, device="cuda")[:, :, :N]
        low = ~upper
        vals[:, low], idx[:, low] = -INF, -1
        st = ops.outcome_topk(x[:3], k, eligible="lower", state=(vals, idx))
        st = ops.outcome_topk(x[3:], k, label_base=3, eligible="lower", state=st)
        assert bool((st[0][:, upper] == MARK_V).all()) and bool((st[1][:, upper] == MARK_I).all())
        assert torch.equal(st[0][:, low], got[0][:, low]) and torch.equal(st[1][:, low], got[1][:, low])


@pytest.mark.parametrize("fresh", [True, False])
@pytest.mark.parametrize("off,width", [(4, 72), (1, 69)])
def test_writes_are_bounded(ops, off, width, fresh):
    """The state embedded in larger marker-filled buffers (a guard plane, guard rows, guard columns on both sides; the 16-byte path
    at column offset 4 and the element path at offset 1): the padding and the surroundings stay unchanged."""
    L, nh, nt, k = 6, 5, 63, 5
    v = _values(L, nh, nt, torch.float32, 9)
    x = _place(ops, v, "pitched")
    big_v = torch.full((k + 2, nh + 2, width), MARK_V, device="cuda")
    big_i = torch.full((k + 2, nh + 2, width), MARK_I, dtype=torch.int32, device="cuda")
    vals, idx = big_v[1:k + 1, 1:nh + 1, off:off + nt], big_i[1:k + 1, 1:nh + 1, off:off + nt]
    for eligible in ("all", "lower"):
        big_v.fill_(MARK_V)
        big_i.fill_(MARK_I)
        if fresh:
            _check(ops, x, v, k, (off, eligible), eligible=eligible)
            st = ops.outcome_topk(x, k, eligible=eligible)
            from madrigal_amd._lib import call                                   # the C entry: a fresh fold into the caller's tensors
            call("mdg_outcome_topk_update", x.data_ptr(), 0, x.stride(0), x.stride(1), None, 0, None, None, vals.data_ptr(), idx.data_ptr(),
                 vals.stride(0), vals.stride(1), nh, nt, L, k, 1, 1, ops.TOPK_ELIGIBLE[eligible], None)
            torch.cuda.synchronize()
            assert torch.equal(vals, st[0]) and torch.equal(idx, st[1])
        else:
            vals.fill_(-INF)
            idx.fill_(-1)
            st = ops.outcome_topk(x, k, eligible=eligible, state=(vals, idx))
            ref = outcome_topk_ref(v, k)
            if eligible == "lower":
                low = (torch.arange(nt)[None, :] < torch.arange(nh)[:, None])
                assert torch.equal(st[0].cpu()[:, low], ref[0][:, low]) and torch.equal(st[1].cpu()[:, low], ref[1][:, low])
            else:
                assert same_state(st, ref)
        inside = torch.zeros_like(big_v, dtype=torch.bool)
        inside[1:k + 1, 1:nh + 1, off:off + nt] = True
        assert bool((big_v[~inside] == MARK_V).all()) and bool((big_i[~inside] == MARK_I).all()), (off, eligible, fresh)


def test_refusals(ops):
    x = torch.randn(4, 6, 6, device="cuda")
    k = 3
    vals, idx = ops.outcome_topk(x, k)
    before = (vals.clone(), idx.clone())                                          # a refused call leaves the state alone
    with pytest.raises(ValueError, match="share one plane stride"):
        ops.outcome_topk(x, k, state=(vals, idx.contiguous()))
    xp = ops.empty_scores(k, 6, 6, "cuda").fill_(1.0)                             # the layout of the state
    with pytest.raises(ValueError, match="alias"):
        ops.outcome_topk(xp, k, state=(xp, idx))
    with pytest.raises(ValueError, match="alias"):
        ops.outcome_topk(x, k, state=(vals, vals.view(torch.int32)))
    for bad in (0, 9):
        with pytest.raises(ValueError, match="k: expected"):
            ops.outcome_topk(x, bad)
    with pytest.raises(ValueError, match="state"):
        ops.outcome_topk(x, 4, state=(vals, idx))                                # the state of another k
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        ops.outcome_topk(x.double(), k)
    with pytest.raises(ValueError, match="state: vals"):
        ops.outcome_topk(x, k, state=(vals.half(), idx))
    with pytest.raises(ValueError, match="state: idx"):
        ops.outcome_topk(x, k, state=(vals, idx.long()))
    with pytest.raises(ValueError, match="labels"):
        ops.outcome_topk(x, k, labels=torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError, match="labels"):
        ops.outcome_topk(x, k, labels=[0, 1, 2])
    with pytest.raises(ValueError, match="label_base"):
        ops.outcome_topk(x, k, label_base=2 ** 31 - 4)
    with pytest.raises(ValueError, match="eligible"):
        ops.outcome_topk(x, k, eligible="not_self")
    with pytest.raises(ValueError, match="unit inner stride"):
        ops.outcome_topk(x.transpose(1, 2), k)
    for bad in (0.0, -1.0, INF, float("nan")):
        with pytest.raises(ValueError, match="scale"):
            ops.outcome_topk(x, k, scale=torch.tensor([1.0, bad, 1.0, 1.0], device="cuda"))
    for bad in (INF, float("nan")):
        with pytest.raises(ValueError, match="shift"):
            ops.outcome_topk(x, k, shift=torch.tensor([1.0, bad, 1.0, 1.0], device="cuda"))
    with pytest.raises(ValueError, match="scale"):
        ops.outcome_topk(x, k, scale=torch.ones(3, device="cuda"))
    with pytest.raises(ValueError, match="shift"):
        ops.outcome_topk(x, k, shift=torch.ones(4))
    assert torch.equal(vals, before[0]) and torch.equal(idx, before[1])
    # empty Nh, Nt or Lc: no launch; a fresh state of no outcome holds the sentinels
    assert ops.outcome_topk(x[:, :0], k)[0].shape == (k, 0, 6) and ops.outcome_topk(x[:, :, :0], k)[1].shape == (k, 6, 0)
    e = ops.outcome_topk(x[:0], k, largest=False)
    assert e[0].shape == (k, 6, 6) and bool((e[0] == INF).all()) and bool((e[1] == -1).all())
    same = ops.outcome_topk(x[:0], k, state=(vals, idx))
    assert torch.equal(same[0], before[0]) and torch.equal(same[1], before[1])


# ------------------------------------------------------------------------------------------------ pipeline level
N_DRUGS, N_OUT, K = 70, 19, 5


@pytest.fixture(scope="module")
def two_models():
    """Two configs.build_model models (drugbank163 layout, 19 outcomes, two seeds) and their embeddings of the same 70 drugs (the
    recipe of tests/test_profile_gpu.py)."""
    from madrigal_amd import configs, data as D, models as M
    from madrigal_amd.pipeline import generate_embeddings
    batch, bkg = D.make_batch(N_DRUGS, 5, kg_nodes=900, kg_edges=6000)
    b = D.batch_to(batch, "cuda")
    kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
    filler = torch.randn((N_DRUGS, 128), generator=torch.Generator().manual_seed(6)).cuda()
    out = []
    for seed in (3, 4):
        torch.manual_seed(seed)
        model = configs.build_model("drugbank163", bkg["data"], N_OUT).cuda().eval()
        with M.precision("bf16x3"):
            z = generate_embeddings(model, b, kgc, kg_filler=filler).contiguous()
        assert z.shape == (N_DRUGS, 128) and bool(torch.isfinite(z).all())
        out.append((model, z))
    return out


def _triple_is(got, ref, k=K):
    vals, idx, mean = got
    assert vals.shape == (k, N_DRUGS, N_DRUGS) and mean.shape == (N_DRUGS, N_DRUGS)
    return same_state((vals, idx), ref) and torch.equal(mean, vals.mean(0))


def test_highest_outcomes_of_a_built_model(ops, two_models):
    """of="ranks" in >= 3 chunks == the reference on rank_normalize(score_all_pairs(...)); the same with 4 outcomes dropped;
    of="scores" with shift / scale == the reference on the dense fp32 scores."""
    from madrigal_amd.pipeline import highest_outcomes, score_all_pairs
    model, z = two_models[0]
    plane = N_DRUGS * ops.empty_scores(1, N_DRUGS, N_DRUGS, "cuda").stride(1) * 4
    with torch.no_grad():
        scores = score_all_pairs(model, z)
        ranks = ops.rank_normalize(scores).cpu()
    ref = outcome_topk_ref(ranks, K)
    assert _triple_is(highest_outcomes(model, z, K, max_bytes=7 * plane), ref)                    # chunks of 7, 7 and 5 outcomes
    assert _triple_is(highest_outcomes(model, z), ref)                                            # one chunk, the defaults
    drop = [2, 7, 8, 18]
    labels = torch.arange(N_OUT)
    labels[drop] = -1
    ref_kept = outcome_topk_ref(ranks, K, labels=labels)
    keep_ids = [l for l in range(N_OUT) if l not in drop]
    assert _triple_is(highest_outcomes(model, z, K, keep=keep_ids, max_bytes=2 * plane), ref_kept)
    assert _triple_is(highest_outcomes(model, z, K, keep=labels >= 0, max_bytes=7 * plane), ref_kept)
    part = highest_outcomes(model, z, 3, label_range=(4, 11), largest=False, max_bytes=3 * plane)
    assert _triple_is(part, outcome_topk_ref(ranks[4:11], 3, label_base=4, largest=False), k=3)
    g = torch.Generator().manual_seed(2)
    shift, scale = torch.randn(N_OUT, generator=g), torch.rand(N_OUT, generator=g) + 0.5
    got = highest_outcomes(model, z, K, of="scores", shift=shift, scale=scale, max_bytes=7 * plane)
    assert _triple_is(got, outcome_topk_ref(scores.cpu(), K, shift=shift, scale=scale))
    with pytest.raises(ValueError, match="of="):
        highest_outcomes(model, z, K, scale=2.0)
    with pytest.raises(ValueError, match="keep"):
        highest_outcomes(model, z, K, keep=[N_OUT])


@pytest.mark.parametrize("np_dtype", [np.float32, np.float16])
def test_highest_outcomes_of_host_arrays_and_memmaps(ops, two_models, tmp_path, np_dtype):
    """highest_outcomes_of from a numpy array and from an np.memmap equals the CUDA-tensor call (and the reference)."""
    from madrigal_amd.pipeline import highest_outcomes_of, rank_all_pairs
    model, z = two_models[0]
    with torch.no_grad():
        ranks = rank_all_pairs(model, z)
    host = ranks.cpu().numpy().astype(np_dtype)
    dev = torch.from_numpy(host).cuda()
    ref = outcome_topk_ref(torch.from_numpy(host), K)
    on_gpu = highest_outcomes_of(dev, K)
    assert _triple_is(on_gpu, ref) and _triple_is(highest_outcomes_of(dev, K, chunk=4), ref)
    mm = np.memmap(tmp_path / "ranks.dat", dtype=np_dtype, mode="w+", shape=host.shape)
    mm[...] = host
    mm.flush()
    ro = np.memmap(tmp_path / "ranks.dat", dtype=np_dtype, mode="r", shape=host.shape)
    labels = np.arange(N_OUT)
    labels[:5] = -1                                                              # the first staged chunk of 4 is skipped whole
    ref_kept = outcome_topk_ref(torch.from_numpy(host), K, labels=labels, eligible="lower")
    for src in (host, ro):
        for chunk in (None, 4):
            got = highest_outcomes_of(src, K, chunk=chunk)
            assert all(torch.equal(a, b) for a, b in zip(got, on_gpu)), (np_dtype, chunk)
        assert _triple_is(highest_outcomes_of(src, K, labels=labels, eligible="lower", chunk=4), ref_kept)
    with pytest.raises(ValueError, match="numpy"):
        highest_outcomes_of(torch.from_numpy(host), K)
    with pytest.raises(ValueError, match="float32 / float16"):
        highest_outcomes_of(host.astype(np.float64), K)


def test_ensemble_highest_outcomes_of_two_seeds(ops, two_models):
    from madrigal_amd.pipeline import ensemble_highest_outcomes, rank_all_pairs
    models, zs = [m for m, _ in two_models], [z for _, z in two_models]
    plane = N_DRUGS * ops.empty_scores(1, N_DRUGS, N_DRUGS, "cuda").stride(1) * 4
    with torch.no_grad():
        ens = ops.ensemble_ranks([rank_all_pairs(m, z) for m, z in zip(models, zs)]).cpu()
    ref = outcome_topk_ref(ens, K)
    assert _triple_is(ensemble_highest_outcomes(models, zs, K, max_bytes=4 * 7 * plane), ref)      # three chunks
    assert _triple_is(ensemble_highest_outcomes(models, zs), ref)
    labels = torch.arange(N_OUT)
    labels[[0, 1, 2, 3, 4, 5, 6, 9]] = -1                                         # the first chunk of 7 is not computed
    got = ensemble_highest_outcomes(models, zs, K, keep=labels >= 0, max_bytes=4 * 7 * plane)
    assert _triple_is(got, outcome_topk_ref(ens, K, labels=labels))
    with pytest.raises(ValueError):
        ensemble_highest_outcomes(models, zs[:1])
