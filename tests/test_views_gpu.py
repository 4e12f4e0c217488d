"""K30 (``fpsg_episode_views``: the uint8 views of an episode -> the encoder's float batch) on the GPU: equal to the numpy
restatement (``_views_ref.py``) bit for bit -- nothing here has a tolerance -- over both kernel forms, every kind of window
and colour triple, the real episode shape and bad ``sel`` entries; ``decode_episode``; and ``trainNetwork.py`` on a tiny
multi-view ModelNet tree."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

import _views_data as vdata
import _views_ref as vref
from fpsg_amd import views

pytestmark = pytest.mark.gpu

SEL = [2, 0, 2, 1, 0]
BIG = 1 << 24
# (x0, y0, step, 0) per image, 1/256 source pixel
GEOMS = {
    "null": None,
    # the identity; step 192; step 300 from negative offsets; fx = fy = 255 throughout; a window left of and above the image
    "a": [(0, 0, 256, 0), (37, 91, 192, 0), (-300, -129, 300, 0), (255, 255, 256, 0), (-5000, -7000, 256, 0)],
    # a window right of and below the image; steps 192 and 300 again; a quarter-pixel step; the limits of the ranges
    "b": [(100000, 90000, 256, 0), (0, 0, 192, 0), (-77, 13, 300, 0), (511, 0, 64, 0), (BIG, -BIG, 65536, 0)],
}
# (brightness, contrast, saturation, 0) per image
COLORS = {
    "null": None,
    "unit": [(0.0, 1.0, 1.0, 0.0)] * 5,
    "mixed": [(0.1, 1.3, 0.5, 0.0), (-0.6, 1.0, 1.0, 0.0), (0.7, 1.5, 1.8, 0.0), (0.0, 1.0, 1.0, 0.0), (-0.05, 0.7, 0.0, 0.0)],
}


def _same(got: torch.Tensor, want: np.ndarray):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    return np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _tables(geom, color):
    return (None if geom is None else torch.tensor(geom, dtype=torch.int32),
            None if color is None else torch.tensor(color, dtype=torch.float32))


@pytest.fixture(scope="module")
def sources():
    rng = np.random.default_rng(30)
    out = {}
    for hs, ws in ((5, 7), (6, 6)):
        src = rng.integers(0, 256, (3, hs, ws, 3), dtype=np.uint8)
        src[0, 0, 0], src[1, -1, -1] = 0, 255                                  # both ends of the byte range
        out[(hs, ws)] = src
    return out


@pytest.mark.parametrize("size", [(4, 4), (8, 8), (7, 5), (8, 12)])          # Wo = 5: the one-pixel form, else four a thread
@pytest.mark.parametrize("shape", [(5, 7), (6, 6)])
def test_equals_the_restatement_bit_for_bit(gpu, sources, shape, size):
    src = sources[shape]
    d_src = torch.from_numpy(src).to(gpu)
    for gname, geom in GEOMS.items():
        for cname, color in COLORS.items():
            want = vref.decode(src, SEL, geom, color, size)
            assert np.isfinite(want).all()
            t_geom, t_color = _tables(geom, color)
            got = views.decode(d_src, torch.tensor(SEL, dtype=torch.int32), t_geom, t_color, size)
            assert tuple(got.shape) == (5, 3) + size
            assert _same(got, want), (shape, size, gname, cname)
            if cname == "mixed":                                               # the triples that clamp do clamp
                assert (want[1] == -1).any() and (want[2] == 1).any()
    # device tables are taken as they are
    t_geom, t_color = _tables(GEOMS["a"], COLORS["mixed"])
    got = views.decode(d_src, torch.tensor(SEL, dtype=torch.int32, device=gpu), t_geom.to(gpu), t_color.to(gpu), size)
    assert _same(got, vref.decode(src, SEL, GEOMS["a"], COLORS["mixed"], size))


def test_windows_outside_the_image_read_the_edge(gpu, sources):
    src = sources[(5, 7)]
    got = views.decode(torch.from_numpy(src).to(gpu), torch.tensor([1, 1], dtype=torch.int32),
                       torch.tensor([GEOMS["a"][4], GEOMS["b"][0]], dtype=torch.int32), None, (8, 12)).cpu().numpy()
    for k, corner in enumerate((src[1, 0, 0], src[1, -1, -1])):                # every tap clamps to one corner pixel
        want = (corner.astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)
        assert np.array_equal(got[k], np.broadcast_to(want[:, None, None], (3, 8, 12)))


def test_the_real_episode_shape(gpu):
    """69 images (a 32-shot episode's), 224 x 224 in and out, a window and a colour triple per image as ``draw`` makes them."""
    rng = np.random.default_rng(69)
    src = rng.integers(0, 256, (69, 224, 224, 3), dtype=np.uint8)
    sel = rng.integers(0, 69, 69).astype(np.int32)
    _, geom, color = views.draw(torch.Generator().manual_seed(5), torch.full((69,), 12), 224, 0.2, 0.4)
    d_src = torch.from_numpy(src).to(gpu)
    got = views.decode(d_src, torch.from_numpy(sel), geom, color)
    assert _same(got, vref.decode(src, sel, geom.numpy(), color.numpy()))
    got = views.decode(d_src, torch.from_numpy(sel))
    assert _same(got, vref.decode(src, sel))


def test_bad_sel_entries_give_nan_images_and_leave_the_others_exact(gpu, sources):
    src = sources[(6, 6)]
    sel = [2, -1, 0, 3, 1]                                                     # -1 and n_src
    t_geom, t_color = _tables(GEOMS["a"], COLORS["mixed"])
    for size in ((8, 8), (7, 5)):
        for geom, color in ((None, None), (t_geom, t_color)):
            # device tensors reach the kernel unchecked; the wrapper raises unless the entry returns 0
            got = views.decode(torch.from_numpy(src).to(gpu), torch.tensor(sel, dtype=torch.int32, device=gpu), geom,
                               color, size)
            want = vref.decode(src, sel, None if geom is None else GEOMS["a"], None if color is None else COLORS["mixed"],
                               size)
            got = got.cpu().numpy()
            for k in (1, 3):
                assert np.isnan(got[k]).all() and np.isnan(want[k]).all()
            for k in (0, 2, 4):
                assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32))
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="sel: entries must be in"):           # a host copy is checked instead
        views.decode(torch.from_numpy(src).to(gpu), torch.tensor(sel, dtype=torch.int32))
    with pytest.raises(ValueError, match="geom: 1 <= step"):
        views.decode(torch.from_numpy(src).to(gpu), torch.tensor([0], dtype=torch.int32),
                     torch.tensor([[0, 0, 0, 0]], dtype=torch.int32))
    with pytest.raises(ValueError, match="geom: .x0"):
        views.decode(torch.from_numpy(src).to(gpu), torch.tensor([0], dtype=torch.int32),
                     torch.tensor([[BIG + 1, 0, 256, 0]], dtype=torch.int32))


def test_decode_episode_on_a_hand_made_sample(gpu):
    rng = np.random.default_rng(3)
    S = 16
    imgs = {k: rng.integers(0, 256, (1, n, S, S, 3), dtype=np.uint8) for k, n in (("xs", 3), ("xq", 2), ("xad", 3))}
    geom = {"xs": [(0, 0, 256, 0), (-40, 300, 200, 0), (700, -90, 290, 0)], "xq": [(5, 5, 256, 0), (0, 0, 256, 0)]}
    color = {"xs": [(0.1, 0.9, 1.2, 0.0), (0.0, 1.0, 1.0, 0.0), (-0.2, 1.4, 0.3, 0.0)]}
    pcs = torch.rand((1, 3, 64, 3), device=gpu)
    sample = {"class": ["cup"], "tmp": torch.tensor([4]), "pcs": pcs}
    for k, x in imgs.items():
        sample[k] = torch.from_numpy(x).to(gpu)
        if k in geom:
            sample[f"{k}_geom"] = torch.tensor(geom[k], dtype=torch.int32)[None]       # collated host tables
        if k in color:
            sample[f"{k}_color"] = torch.tensor(color[k], dtype=torch.float32)[None]
    out = views.decode_episode(sample)
    assert out is sample and set(sample) == {"class", "tmp", "pcs", "xs", "xq", "xad"} and sample["pcs"] is pcs
    for k, x in imgs.items():
        n = x.shape[1]
        want = vref.decode(x[0], np.arange(n), geom.get(k), color.get(k))
        assert tuple(sample[k].shape) == (1, n, 3, S, S) and sample[k].is_contiguous()
        assert _same(sample[k][0], want), k
    # a sample of the default datasets passes through untouched
    floats = {"xs": sample["xs"], "xq": sample["xq"], "xad": sample["xad"], "pcs": pcs}
    again = views.decode_episode(dict(floats))
    assert all(again[k] is v for k, v in floats.items())


# ---- trainNetwork.py ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return vdata.modelnet_tree(tmp_path_factory.mktemp("modelnet"))


# trainNetwork.py seeds its episodes per epoch but not its initial weights, and the ModelNet reader pads short clouds from
# numpy's global stream: two runs print the same losses only from the same seeds, so the runs below start from this launcher
_SEEDED = ("import trainNetwork, numpy, torch; torch.manual_seed(0); numpy.random.seed(0); "
           "trainNetwork.main(trainNetwork.cli.few_shot_parser().parse_args())")


def _train(tree, where, name, extra):
    cfg, aux = tree
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _SEEDED, "--config_path", cfg, "--test_path", cfg, "--refer_path", aux,
                        "--n_shot", "2", "--n_query", "1", "--intra_recon", "--epoch", "2", "--n_episode", "2",
                        "--eval_interval", "9", "--sample_interval", "9", "--model_path", str(where), "--name", name]
                       + extra, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("Training Results for Epoch")]
    assert len(lines) == 2, r.stdout[-3000:]
    for ln in lines:
        m = re.search(r"Query_rec: (\S+), Support_rec: (\S+)$", ln)
        assert m, ln
        assert all(math.isfinite(float(v)) and float(v) > 0.0 for v in m.groups()), ln
    assert os.path.exists(os.path.join(str(where), name, "model_epoch_2.pt"))
    return lines


def test_training_on_all_views_with_both_jitters(gpu, tree, tmp_path):
    _train(tree, tmp_path, "v", ["--n_views", "0", "--view_jitter", "0.1", "--view_color_jitter", "0.2"])


def test_one_view_without_jitter_trains_as_without_the_options(gpu, tree, tmp_path):
    plain = _train(tree, tmp_path, "p", [])
    same = _train(tree, tmp_path, "s", ["--n_views", "1", "--view_jitter", "0", "--view_color_jitter", "0"])
    assert same == plain
