"""Training on all rendered views (``fpsg_amd.views``, K30), what needs no GPU: the numpy restatement (``_views_ref.py``)
against today's image pipeline, the uint8 view corpora against today's float corpora, the episode indices and the global
random stream with views on, ``views.draw``, the three options and their refusals, and the C entry's host refusals."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import _views_data as vdata
import _views_ref as vref
from fpsg_amd import cli, datasets, views
from fpsg_amd._hip import FpsgHipError


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """dataset -> ((config file, auxiliary dir), default class, multi-view class, transform): one tiny tree each."""
    return {"modelnet": (vdata.modelnet_tree(tmp_path_factory.mktemp("modelnet")), datasets.FewShotModelNet,
                         views.MultiViewModelNet, datasets.modelnet_transform()),
            "shapenet": (vdata.shapenet_tree(tmp_path_factory.mktemp("shapenet")), datasets.FewShotShapeNet,
                         views.MultiViewShapeNet, datasets.shapenet_transform())}


def _build(cls, paths, tfs, **kw):
    np.random.seed(5)                                   # the ShapeNet reader subsamples its clouds from numpy's stream
    return cls(paths[0], paths[1], n_classes=1, n_support=2, n_query=2, transform=tfs, **kw)


# ---- the restatement against today's pipeline -------------------------------------------------------------------------

@pytest.mark.parametrize("crop", [550, 256])
@pytest.mark.parametrize("size", [(600, 600), (640, 580), (300, 200)])     # square, not square, smaller than the crop
def test_restatement_without_tables_is_todays_image_transform(crop, size):
    rng = np.random.default_rng(size[0] + crop)
    img = Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8))
    tfs = datasets.ImageTransform(crop)
    want = tfs(img).numpy()
    pixels = tfs.to_uint8(img)
    assert pixels.dtype == np.uint8 and pixels.shape == (224, 224, 3)
    got = vref.decode(pixels[None], [0])
    assert got.dtype == np.float32 and got.shape == (1, 3, 224, 224)
    assert np.array_equal(got[0].view(np.uint32), want.view(np.uint32))


def test_restatement_at_zero_fractions_is_p_over_255_for_every_byte():
    p = np.arange(256, dtype=np.uint8)
    src = np.broadcast_to(p[None, :, None, None], (1, 256, 2, 3)).copy()
    got = vref.decode(src, [0])[0, 0, :, 0]
    want = (p.astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- corpora ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["modelnet", "shapenet"])
def pair(request, trees):
    """(default dataset, multi-view dataset with --n_views 0 --view_jitter 0.2) over one tiny tree."""
    paths, cls, many, tfs = trees[request.param]
    return _build(cls, paths, tfs), _build(many, paths, tfs, n_views=0, view_jitter=0.2)


def test_view_zero_of_the_corpus_is_todays_float_corpus(pair):
    default, multi = pair
    corpus = multi.view_corpus
    assert isinstance(corpus, views.ViewCorpus) and corpus.images.dtype == torch.uint8
    assert tuple(corpus.images.shape) == (10, 3, 224, 224, 3) and corpus.V == 3 and len(corpus) == 10
    short = vdata.SHORT[0] * vdata.ITEMS + vdata.SHORT[1]
    assert corpus.counts.dtype == torch.int32
    assert corpus.counts.tolist() == [2 if i == short else 3 for i in range(10)]
    assert not corpus.images[short, 2].any()                                   # an unused slot
    first = corpus[:, 0].numpy()
    got = vref.decode(first, np.arange(10))
    assert np.array_equal(got.view(np.uint32), default.img_corpus.numpy().view(np.uint32))
    assert torch.equal(multi.pc_corpus, default.pc_corpus)
    assert list(multi.reference) == list(default.reference)
    start = 0
    for name, entry in default.reference.items():
        mine = multi.reference[name]
        assert torch.equal(mine["pcs"], entry["pcs"])
        assert torch.equal(mine["views"].images, corpus.images[start:start + len(entry["imgs"])])
        assert mine["views"].images.data_ptr() == corpus.images[start].data_ptr()       # a slice, not a copy
        start += len(entry["imgs"])
    # the views differ from one another, and rows() is the [items * V] view the episodes gather from
    assert not torch.equal(corpus[0, 0], corpus[0, 1])
    assert torch.equal(corpus.rows()[4 * 3 + 2], corpus[4, 2])


def test_n_views_limits_the_slots(trees):
    paths, _, many, tfs = trees["shapenet"]
    two, full = _build(many, paths, tfs, n_views=2), _build(many, paths, tfs, n_views=0)
    assert tuple(two.view_corpus.images.shape) == (10, 2, 224, 224, 3) and two.view_corpus.counts.tolist() == [2] * 10
    assert torch.equal(two.view_corpus.images, full.view_corpus.images[:, :2])
    before = two[3]["xs"].shape
    assert two.to(torch.device("cpu")) is two and two[3]["xs"].shape == before             # to(): the corpora and their slices
    assert all(e["views"].images.data_ptr() >= two.view_corpus.images.data_ptr() for e in two.reference.values())


def _episodes(ds, monkeypatch, n=10):
    """``n`` episodes under one seed: every permutation drawn from the global stream, ``tmp``, the clouds, the samples
    and the global generator's state afterwards."""
    drawn = []
    inner = torch.randperm

    def spy(*a, **k):
        out = inner(*a, **k)
        drawn.append(out.clone())
        return out

    monkeypatch.setattr(torch, "randperm", spy)
    torch.manual_seed(11)
    order = torch.randperm(len(ds))[:n].tolist()
    samples = [ds[i] for i in order]
    monkeypatch.setattr(torch, "randperm", inner)
    return drawn, samples, torch.get_rng_state()


def test_indices_tmp_and_the_global_stream_do_not_change_with_views_on(pair, monkeypatch):
    default, multi = pair
    multi.seed_views(3)
    d_drawn, d_samples, d_state = _episodes(default, monkeypatch)
    m_drawn, m_samples, m_state = _episodes(multi, monkeypatch)
    assert len(d_drawn) == len(m_drawn) == 1 + 2 * 10                          # per episode: the class's, then the "ad"
    assert all(torch.equal(a, b) for a, b in zip(d_drawn, m_drawn))
    assert torch.equal(d_state, m_state)
    corpus = multi.view_corpus
    rows = corpus.rows()
    for n, (a, b) in enumerate(zip(d_samples, m_samples)):
        assert a["class"] == b["class"] and a["tmp"] == b["tmp"]
        for key in ("pcs", "pcq", "pcad"):
            assert torch.equal(a[key], b[key])
        ad = m_drawn[2 + 2 * n][:2]
        for key, n_img in (("xs", 2), ("xq", 2), ("xad", 2)):
            x, geom = b[key], b[f"{key}_geom"]
            assert x.dtype == torch.uint8 and tuple(x.shape) == (n_img, 224, 224, 3)
            assert geom.dtype == torch.int32 and tuple(geom.shape) == (n_img, 4) and f"{key}_color" not in b
            assert x.reshape(n_img, -1).any(dim=1).all()                       # never an unused slot
        # the "ad" images are views of the items the "ad" permutation names
        for k in range(2):
            item = int(ad[k])
            assert any(torch.equal(b["xad"][k], rows[item * corpus.V + v]) for v in range(int(corpus.counts[item])))
        assert set(b) == set(a) | {"xs_geom", "xq_geom", "xad_geom"}


def test_seed_views_repeats_the_views_and_only_them(pair, monkeypatch):
    _, multi = pair
    multi.seed_views(7)
    _, first, _ = _episodes(multi, monkeypatch, n=3)
    multi.seed_views(7)
    _, again, _ = _episodes(multi, monkeypatch, n=3)
    multi.seed_views(8)
    _, other, _ = _episodes(multi, monkeypatch, n=3)
    for a, b in zip(first, again):
        assert all(torch.equal(a[k], b[k]) for k in ("xs", "xq", "xad", "xs_geom", "xq_geom", "xad_geom"))
    assert any(not torch.equal(a["xs_geom"], b["xs_geom"]) for a, b in zip(first, other))
    assert all(torch.equal(a["pcs"], b["pcs"]) for a, b in zip(first, other))


def test_colour_tables_come_with_colour_jitter_and_collate_keeps_them(trees):
    from fpsg_amd.episodes import collate_episode
    paths, _, many, tfs = trees["shapenet"]
    ds = _build(many, paths, tfs, n_views=1, view_color_jitter=0.3)
    assert ds.view_corpus.V == 1
    sample = collate_episode(ds[0])
    for key in views.IMAGE_KEYS:
        assert tuple(sample[key].shape) == (1, 2, 224, 224, 3) and sample[key].dtype == torch.uint8
        assert sample[f"{key}_geom"].dtype == torch.int32 and tuple(sample[f"{key}_geom"].shape) == (1, 2, 4)
        assert (sample[f"{key}_geom"][0] == torch.tensor([0, 0, 256, 0], dtype=torch.int32)).all()
        color = sample[f"{key}_color"][0]
        assert color.dtype == torch.float32 and tuple(color.shape) == (2, 4)
        assert (color[:, 0].abs() <= 0.075).all() and ((color[:, 1:3] - 1).abs() <= 0.3).all() and (color[:, 3] == 0).all()
    with pytest.raises(FpsgHipError, match="no CPU fallback"):
        views.decode_episode(sample)                                           # the images are on the host


# ---- views.draw ---------------------------------------------------------------------------------------------------------

def test_draw_without_jitter_gives_identity_tables_and_no_colour_table():
    g = torch.Generator().manual_seed(0)
    counts = torch.tensor([3, 1, 2, 12, 3], dtype=torch.int32)
    view, geom, color = views.draw(g, counts, 224, 0.0, 0.0)
    assert color is None and view.dtype == torch.int64 and geom.dtype == torch.int32
    assert geom.tolist() == [[0, 0, 256, 0]] * 5
    assert view[1] == 0 and (view >= 0).all() and (view < counts).all()


def test_drawn_views_stay_below_each_items_count_and_reach_every_view():
    g = torch.Generator().manual_seed(1)
    counts = torch.tensor([1, 2, 3, 12] * 500)
    view, _, _ = views.draw(g, counts, 224, 0.3, 0.5)
    assert (view >= 0).all() and (view < counts).all()
    for c in (1, 2, 3, 12):
        assert sorted(set(view[counts == c].tolist())) == list(range(c))


@pytest.mark.parametrize("J, C", [(0.0, 0.0), (0.2, 0.0), (0.0, 0.4), (0.49, 0.99)])
def test_draw_is_its_restatement_and_repeats_under_a_seed(J, C):
    counts = torch.tensor([3, 3, 2, 1, 12, 7, 3])
    view, geom, color = views.draw(torch.Generator().manual_seed(42), counts, 224, J, C)
    view2, geom2, color2 = views.draw(torch.Generator().manual_seed(42), counts, 224, J, C)
    assert torch.equal(view, view2) and torch.equal(geom, geom2)
    assert (color is None and color2 is None) or torch.equal(color, color2)
    u = torch.rand(7, 7, dtype=torch.float64, generator=torch.Generator().manual_seed(42)).numpy()
    rview, rgeom, rcolor = vref.draw(u, counts.numpy(), 224, J, C)
    assert np.array_equal(view.numpy(), rview) and np.array_equal(geom.numpy(), rgeom)
    if C == 0:
        assert color is None and rcolor is None
    else:
        assert np.array_equal(color.numpy().view(np.uint32), rcolor.view(np.uint32))
        assert (color[:, 0].abs() <= C / 4).all() and ((color[:, 1:3] - 1).abs() <= C + 1e-6).all()
    # the window: its side within 1 -+ J of the image's, its centre within J / 2 of the side off the middle
    step, S = geom[:, 2].double(), 224
    assert ((step - 256).abs() <= 256 * J + 0.5).all() and (geom[:, 3] == 0).all()
    for axis in (0, 1):
        centre = (geom[:, axis].double() + (S - 1) * step / 2) / 256
        assert ((centre - (S - 1) / 2).abs() <= S * J / 2 + 1 / 256).all()
    assert views.MAX_OFFSET >= int(geom[:, :2].abs().max()) and 1 <= int(geom[:, 2].min())


def test_draw_never_touches_the_global_generator():
    torch.manual_seed(0)
    before = torch.get_rng_state()
    views.draw(torch.Generator().manual_seed(1), torch.tensor([3, 3]), 224, 0.1, 0.1)
    assert torch.equal(before, torch.get_rng_state())


# ---- options ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("evaluation", [False, True])
def test_parser_defaults_and_types(evaluation):
    p = cli.few_shot_parser(evaluation=evaluation)
    base = vars(p.parse_args([]))
    assert base["n_views"] == 1 and type(base["n_views"]) is int
    assert base["view_jitter"] == 0.0 and type(base["view_jitter"]) is float
    assert base["view_color_jitter"] == 0.0 and type(base["view_color_jitter"]) is float
    on = vars(p.parse_args(["--n_views", "0", "--view_jitter", "0.2", "--view_color_jitter", "0.3"]))
    assert (on["n_views"], on["view_jitter"], on["view_color_jitter"]) == (0, 0.2, 0.3)
    mine = {"n_views", "view_jitter", "view_color_jitter"}
    assert {k: v for k, v in on.items() if k not in mine} == {k: v for k, v in base.items() if k not in mine}
    group = next(g for g in p._action_groups if g.title == "data / episode")
    assert mine <= {a.dest for a in group._group_actions}


_FILES = ["--config_path", "a.txt", "--test_path", "b.txt"]


@pytest.mark.parametrize("flag, bad, text", [
    ("n_views", -1, "--n_views must be an integer >= 0"),
    ("n_views", 1.5, "--n_views must be an integer >= 0"),
    ("n_views", True, "--n_views must be a number"),
    ("n_views", "3", "--n_views must be a number"),
    ("view_jitter", -0.1, "--view_jitter must be in [0, 0.5)"),
    ("view_jitter", 0.5, "--view_jitter must be in [0, 0.5)"),
    ("view_jitter", float("nan"), "--view_jitter must be a number"),
    ("view_jitter", False, "--view_jitter must be a number"),
    ("view_jitter", "x", "--view_jitter must be a number"),
    ("view_color_jitter", -0.5, "--view_color_jitter must be in [0, 1)"),
    ("view_color_jitter", 1.0, "--view_color_jitter must be in [0, 1)"),
    ("view_color_jitter", float("inf"), "--view_color_jitter must be in [0, 1)"),
    ("view_color_jitter", True, "--view_color_jitter must be a number"),
    ("view_color_jitter", None, "--view_color_jitter must be a number"),
])
def test_validate_refuses_bad_values_and_names_the_flag(flag, bad, text):
    p = cli.few_shot_parser()
    cli.validate(p.parse_args(_FILES + ["--n_views", "0", "--view_jitter", "0.49", "--view_color_jitter", "0.99"]))
    cli.validate(p.parse_args(_FILES))
    opt = p.parse_args(_FILES)
    setattr(opt, flag, bad)
    with pytest.raises(SystemExit) as e:
        cli.validate(opt)
    assert str(e.value).startswith(text), str(e.value)


@pytest.mark.parametrize("argv, flag", [(["--n_views", "0"], "--n_views"), (["--n_views", "3"], "--n_views"),
                                        (["--view_jitter", "0.1"], "--view_jitter"),
                                        (["--view_color_jitter", "0.1"], "--view_color_jitter")])
def test_validate_refuses_the_options_with_synthetic_corpora(argv, flag):
    p = cli.few_shot_parser()
    cli.validate(p.parse_args(["--synthetic", "--n_views", "1", "--view_jitter", "0", "--view_color_jitter", "0"]))
    with pytest.raises(SystemExit) as e:
        cli.validate(p.parse_args(["--synthetic"] + argv))
    assert str(e.value).startswith(f"{flag} ") and "--synthetic" in str(e.value)


def test_validate_passes_a_namespace_from_before_the_options():
    opt = cli.few_shot_parser().parse_args(["--synthetic"])
    for name in ("n_views", "view_jitter", "view_color_jitter"):
        delattr(opt, name)
    cli.validate(opt)
    assert cli.multi_view(opt) is False


@pytest.mark.parametrize("dataset", ["modelnet", "shapenet"])
def test_build_datasets_default_options_give_todays_classes_and_views_only_train(trees, dataset):
    (cfg, aux), cls, many, _ = trees[dataset]
    argv = ["--config_path", cfg, "--test_path", cfg, "--refer_path", aux, "--n_shot", "2", "--n_query", "2",
            "--dataset", dataset]
    p = cli.few_shot_parser()
    ds, ds_test = cli.build_datasets(p.parse_args(argv), 2, torch.device("cpu"))
    assert type(ds) is cls and type(ds_test) is cls
    same = p.parse_args(argv + ["--n_views", "1", "--view_jitter", "0", "--view_color_jitter", "0"])
    ds, ds_test = cli.build_datasets(same, 2, torch.device("cpu"))
    assert type(ds) is cls and type(ds_test) is cls
    on = p.parse_args(argv + ["--n_views", "0", "--view_color_jitter", "0.2"])
    ds, ds_test = cli.build_datasets(on, 2, torch.device("cpu"))
    assert type(ds) is many and type(ds_test) is cls
    assert (ds.n_views, ds.view_jitter, ds.view_color_jitter) == (0, 0.0, 0.2) and ds.view_corpus.V == 3
    assert not hasattr(ds, "img_corpus")                                       # no float images are kept
    ds, ds_test = cli.build_datasets(on, 2, torch.device("cpu"), views=False)  # what evaluate_Network.py asks for
    assert type(ds) is cls and type(ds_test) is cls


# ---- the wrapper and the C entry ----------------------------------------------------------------------------------------

def test_decode_has_no_cpu_fallback():
    with pytest.raises(FpsgHipError, match="no CPU fallback"):
        views.decode(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32))


@pytest.fixture(scope="module")
def lib():
    from fpsg_amd import _hip
    assert "fpsg_episode_views" in _hip.SIGNATURES
    return _hip.load()


def test_entry_refuses_on_the_host_before_any_hip_call(lib):
    f = lib.fpsg_episode_views
    fake = ctypes.c_void_p(64)                                                 # non-null, aligned, never dereferenced

    def call(src=None, n_src=3, Hs=5, Ws=7, sel=None, n=5, geom=None, color=None, out=None, Ho=4, Wo=4):
        return f(src, n_src, Hs, Ws, sel, n, geom, color, out, Ho, Wo, None)

    assert call() == -1 and b"null pointer 'src'" in lib.fpsg_last_error()
    assert call(src=fake) == -1 and b"null pointer 'sel'" in lib.fpsg_last_error()
    assert call(src=fake, sel=fake) == -1 and b"null pointer 'out'" in lib.fpsg_last_error()
    for name in ("n_src", "Hs", "Ws", "n", "Ho", "Wo"):
        for bad in (0, -1):
            assert call(**{name: bad}) == -2 and b"must be positive" in lib.fpsg_last_error(), name
    for name in ("Hs", "Ws", "Ho", "Wo"):
        assert call(**{name: views.MAX_SIZE + 1}) == -4 and b"<= 8192" in lib.fpsg_last_error(), name
        assert call(**{name: views.MAX_SIZE}) == -1                            # the limit itself passes the shape checks
    assert call(n=views.MAX_IMAGES + 1) == -4 and call(n=views.MAX_IMAGES) == -1
    odd = ctypes.c_void_p(66)
    assert call(src=fake, sel=odd, out=fake) == -3
    assert call(src=fake, sel=fake, out=odd) == -3
    assert call(src=fake, sel=fake, out=fake, geom=odd) == -3 and call(src=fake, sel=fake, out=fake, color=odd) == -3
    assert call(src=odd) == -1 and b"'sel'" in lib.fpsg_last_error()           # bytes: src needs no alignment
