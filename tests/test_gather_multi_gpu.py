"""ops.gather_rows_multi (mdg_gather_rows_multi): rows gathered across several matrices are, bit for bit, the rows of
torch.cat(sources).index_select(0, idx); the optional operand image has the bytes of ops.pack_operand on them; and the encoder
computes the same embeddings whether it reads its tx / uni-modal / KG rows through the kernel or through the stacked copies."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _sources(n_src, rows, width, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(rows, width, generator=g).cuda() for _ in range(n_src)]


def _index(kind, total, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "empty":
        return torch.zeros(0, dtype=torch.int64)
    if kind == "one":
        return torch.tensor([total - 1], dtype=torch.int64)
    if kind == "shuffled_repeated":                     # out of order, every third row twice, a count that is no multiple of 64 or 256
        idx = torch.randperm(total, generator=g)[: max(1, (2 * total) // 3)]
        idx = torch.cat([idx, idx[::3]])
        return idx[torch.randperm(idx.numel(), generator=g)][: idx.numel() - (idx.numel() % 64 == 0)]
    raise ValueError(kind)


@pytest.mark.parametrize("width", [128, 978])
@pytest.mark.parametrize("n_src", [1, 3, 16])
@pytest.mark.parametrize("kind", ["empty", "one", "shuffled_repeated"])
def test_rows_equal_cat_index_select(n_src, width, kind):
    from madrigal_amd import ops
    rows = 37
    srcs = _sources(n_src, rows, width, 100 + n_src)
    idx = _index(kind, n_src * rows, 7).cuda()
    want = torch.cat(srcs).index_select(0, idx)
    got = ops.gather_rows_multi(srcs, idx)
    assert got.shape == want.shape and torch.equal(got, want)
    padded = ops.gather_rows_multi(srcs, idx, pad4=True)
    w4 = (width + 3) // 4 * 4
    assert padded.shape == (idx.numel(), w4) and padded.is_contiguous()
    assert torch.equal(padded[:, :width], want) and bool((padded[:, width:] == 0).all())


@pytest.mark.parametrize("width", [128, 978, 131])
def test_unaligned_sources_and_row_views(width):
    """Sources that start 4 or 8 bytes off a 16-byte boundary, or are row slices / column-strided views of larger matrices."""
    from madrigal_amd import ops
    rows = 21
    g = torch.Generator().manual_seed(3)
    flat = torch.randn(3 * rows * (width + 8) + 8, generator=g).cuda()
    a = flat[1: 1 + rows * width].view(rows, width)                                   # 4 bytes off
    b = flat[rows * width + 2: 2 + 2 * rows * width].view(rows, width)                # 8 bytes off
    big = torch.randn(rows + 5, width + 8, generator=g).cuda()
    c = big[3: 3 + rows, 4: 4 + width]                                                # row stride width + 8
    idx = torch.randperm(3 * rows, generator=g).cuda()
    want = torch.cat([a, b, c]).index_select(0, idx)
    assert torch.equal(ops.gather_rows_multi([a, b, c], idx), want)


def test_short_sources_and_indices_outside_them_give_zero_rows():
    """rows_per_source larger than the sources (the KG rows beside the filler table): an index past its source's rows, past the last
    source, or negative gathers zeros and nothing else is read."""
    from madrigal_amd import ops
    g = torch.Generator().manual_seed(5)
    a, b = torch.randn(5, 128, generator=g).cuda(), torch.randn(9, 128, generator=g).cuda()
    idx = torch.tensor([0, 4, 5, 9, 10, 18, 19, 25, -1, 12], dtype=torch.int64).cuda()          # rows_per_source = 10
    got = ops.gather_rows_multi([a, b], idx, rows_per_source=10)
    zero = torch.zeros(128).cuda()
    want = torch.stack([a[0], a[4], zero, zero, b[0], b[8], zero, zero, zero, b[2]])
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        ops.gather_rows_multi([a, b], idx)                   # different row counts need rows_per_source
    with pytest.raises(ValueError):
        ops.gather_rows_multi([a] * 20, idx, rows_per_source=10)


@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
@pytest.mark.parametrize("width", [128, 978])
def test_image_has_the_bytes_of_pack_operand(width, precision):
    from madrigal_amd import ops
    srcs = _sources(3, 37, width, 11)
    idx = _index("shuffled_repeated", 3 * 37, 9).cuda()
    want_rows = torch.cat(srcs).index_select(0, idx)
    want_img = ops.pack_operand(want_rows, precision)
    rows, img = ops.gather_rows_multi(srcs, idx, image=precision)
    assert torch.equal(rows, want_rows)
    kp = (width + 63) // 64 * 64
    used = idx.numel() * kp * (4 if precision == "bf16x3" else 2)          # (the allocation is rounded up to 256 bytes behind the image)
    assert img.numel() == want_img.numel() and used <= img.numel()
    assert torch.equal(img[:used], want_img[:used])
    none_rows, img2 = ops.gather_rows_multi(srcs, idx, image=precision, want_fp32=False)
    assert none_rows is None and torch.equal(img2[:used], want_img[:used])
    # the dense block takes it as it takes pack_operand's (weight zero-padded to the image's inner length)
    w = torch.randn(64, width, generator=torch.Generator().manual_seed(2)).cuda()
    wk = torch.nn.functional.pad(w, (0, kp - width)).contiguous()
    y = ops.linear_packed(img, idx.numel(), wk, precision=precision)
    assert torch.equal(y, ops.linear_packed(want_img, idx.numel(), wk, precision=precision))
    ref = want_rows.double() @ w.double().t()
    assert float((y.double() - ref).abs().max() / ref.abs().max()) < (1e-4 if precision == "bf16x3" else 3e-2)
    rows32, img32 = ops.gather_rows_multi(srcs, idx, image="f32")            # the fp32 mode takes the rows themselves
    assert img32 is None and torch.equal(rows32, want_rows)


def test_encoder_is_bit_identical_with_and_without_the_gathers():
    """encoder(...) at 64 drugs over a KG of 800 nodes / 9 000 edges: reading the present tx signatures, the uni-modal rows and the
    batch's KG rows through the gather kernel gives torch.equal embeddings to the stacked copies (the composed last KG conv, where a
    model has that switch, off in both calls)."""
    from madrigal_amd import configs, data as D, models as M
    from oracle.params import det_state_dict
    n = 64
    batch, bkg = D.make_batch(n, 5, kg_nodes=800, kg_edges=9000)
    model = configs.build_model("twosides321", bkg["data"], 7)
    sd = model.state_dict()
    skip = [k for k in sd if k.endswith("pos_encoder.pe")]
    model.load_state_dict({**sd, **det_state_dict(3, {k: tuple(v.shape) for k, v in sd.items()}, skip)})
    model = model.cuda().eval()
    for mod in model.modules():
        if hasattr(mod, "fold_wanted"):
            mod.fold_wanted = False
    enc = model.encoder
    b = D.batch_to(batch, "cuda")
    kgc = {"data": bkg["data"].to("cuda"), "drug_index_map": bkg["drug_index_map"].cuda()}
    filler = torch.randn(n, 128, generator=torch.Generator().manual_seed(6)).cuda()
    mp = enc._mask_plan(b["masks"], torch.device("cuda", torch.cuda.current_device()), True)
    assert mp["n_uni"] > 0 and 0 < mp["tx_rows"].numel() < 16 * n          # the batch has uni-modal drugs and absent signatures
    assert bool(b["masks"][:, 1].any()) and not bool(b["masks"][:, 1].all())   # drugs inside and outside the KG

    def run(on):
        enc.gather_tx_rows = enc.gather_uni_rows = enc.gather_kg_rows = on
        with torch.no_grad(), M.precision("bf16x3"):
            return enc(b["drugs"], b["masks"], b["strs"], kgc, b["cv"], b["tx"], kg_filler=filler)

    z_on, z_off, z_on2 = run(True), run(False), run(True)
    assert z_on.shape == (n, 128) and bool(torch.isfinite(z_on).all())
    assert torch.equal(z_on, z_off) and torch.equal(z_on, z_on2)
    for name in ("gather_tx_rows", "gather_uni_rows", "gather_kg_rows"):          # each switch alone
        enc.gather_tx_rows = enc.gather_uni_rows = enc.gather_kg_rows = False
        setattr(enc, name, True)
        with torch.no_grad(), M.precision("bf16x3"):
            assert torch.equal(enc(b["drugs"], b["masks"], b["strs"], kgc, b["cv"], b["tx"], kg_filler=filler), z_off), name
