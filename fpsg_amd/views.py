"""Training on all rendered views: uint8 view corpora and their decode on the GPU (K30, ``fpsg_episode_views``).

``prepare_dataset.py`` renders several views of every item; the default datasets read one.  Here a corpus keeps up to
``V`` views per item as the uint8 pixels PIL produced (147 KB an image instead of the 602 KB of its normalised floats),
an episode draws a view per image -- and, optionally, a crop window and a colour jitter -- from a generator of its own,
gathers the uint8 rows, and one K30 launch per image tensor turns them into the float batch the encoder reads, after the
upload, on the current stream.  ``decode`` runs on the GPU only: a CPU tensor raises ``FpsgHipError`` (no CPU fallback).

The episode's support, query and "ad" indices come from the same ``torch.randperm`` calls in the same order as in the
default datasets (``tests/golden/episode_streams.npz``); everything view-related is drawn from the datasets' own generator
(``seed_views``), so an epoch's episodes do not change because views are on.  All of it is opt-in: ``--n_views``,
``--view_jitter``, ``--view_color_jitter`` (``cli.build_datasets``); evaluation always reads view 0.
"""
from __future__ import annotations

import os

import numpy as np
import torch
from PIL import Image

from . import _hip
from .datasets import FewShotModelNet, FewShotShapeNet, to_unit_ball
from .episodes import take_rows

MAX_SIZE = 8192                 # FPSG_VIEWS_MAX_SIZE
MAX_IMAGES = 65535              # FPSG_VIEWS_MAX_IMAGES
MAX_OFFSET = 1 << 24            # FPSG_VIEWS_MAX_OFFSET
MAX_STEP = 1 << 16              # FPSG_VIEWS_MAX_STEP
IMAGE_KEYS = ("xs", "xq", "xad")


# ------------------------------------------------------------------------------------- options
def _number(value, flag):
    if isinstance(value, bool) or not isinstance(value, (int, float)) or value != value:
        raise ValueError(f"{flag} must be a number, got {value!r}")
    return value


def check_view_options(n_views, view_jitter, view_color_jitter, synthetic: bool = False) -> bool:
    """``--n_views`` (an integer >= 0, 0 = all views found), ``--view_jitter`` in [0, 0.5), ``--view_color_jitter`` in
    [0, 1); none of them with synthetic corpora (``ValueError`` naming the flag otherwise).  True when any of them is
    away from its default, i.e. when training reads a multi-view dataset."""
    _number(n_views, "n_views")
    if not isinstance(n_views, int) or n_views < 0:
        raise ValueError(f"n_views must be an integer >= 0 (0 = all views found), got {n_views!r}")
    if not 0.0 <= _number(view_jitter, "view_jitter") < 0.5:
        raise ValueError(f"view_jitter must be in [0, 0.5), got {view_jitter!r}")
    if not 0.0 <= _number(view_color_jitter, "view_color_jitter") < 1.0:
        raise ValueError(f"view_color_jitter must be in [0, 1), got {view_color_jitter!r}")
    for flag, on in (("n_views", n_views != 1), ("view_jitter", view_jitter != 0),
                     ("view_color_jitter", view_color_jitter != 0)):
        if on and synthetic:
            raise ValueError(f"{flag} reads rendered views from files; it cannot be combined with --synthetic")
    return n_views != 1 or view_jitter != 0 or view_color_jitter != 0


# ------------------------------------------------------------------------------------- K30
def _table(t, dtype, shape, name, src):
    """A per-image table as a device tensor.  A host copy is range-checked first and uploaded; a device
    tensor is taken as it is (the kernel clamps ``geom`` and answers a bad ``sel`` entry with NaNs)."""
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t), dtype=dtype)
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if tuple(t.shape) != shape:
        raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
    if t.device.type == "cpu":
        if name == "sel" and t.numel() and not (0 <= int(t.min()) and int(t.max()) < src.shape[0]):
            raise ValueError(f"sel: entries must be in [0, {src.shape[0]}), got {int(t.min())}..{int(t.max())}")
        if name == "geom":
            if int(t[:, :2].abs().max()) > MAX_OFFSET:
                raise ValueError(f"geom: |x0|, |y0| <= {MAX_OFFSET} (1/256 pixel) are supported")
            if not (1 <= int(t[:, 2].min()) and int(t[:, 2].max()) <= MAX_STEP):
                raise ValueError(f"geom: 1 <= step <= {MAX_STEP} (1/256 pixel) is supported")
        if name == "color" and not bool(torch.isfinite(t).all()):
            raise ValueError("color: brightness, contrast and saturation must be finite")
        t = t.contiguous().to(src.device, non_blocking=True)
    return _hip.dev_tensor(t, dtype, name)


def decode(src: torch.Tensor, sel, geom=None, color=None, size=None) -> torch.Tensor:
    """K30: uint8 images ``src [n_src,Hs,Ws,3]`` (HWC) -> float32 ``[n,3,Ho,Wo]``, image ``k`` made from ``src[sel[k]]``
    through the window ``geom[k] = (x0, y0, step, 0)`` (int32, 1/256 source pixel; None: the identity ``(0, 0, 256)``), the
    photometric step ``color[k] = (brightness, contrast, saturation, 0)`` (float32; None: no such step) and
    ``(x - 0.5) / 0.5``.  ``size``: ``Ho`` or ``(Ho, Wo)``, default the source's.  ``include/fpsg_hip.h`` (K30) has the
    definition; ``tests/_views_ref.py`` restates it.

    ``src`` lives on the GPU (``FpsgHipError`` otherwise).  ``sel``, ``geom`` and ``color`` may be host tensors: their
    ranges are checked here (``ValueError``) and they are uploaded; device tensors go to the kernel unchecked, which
    clamps ``geom`` to its ranges and writes an image of NaNs for a ``sel`` entry outside ``[0, n_src)``."""
    _hip.dev_tensor(src, torch.uint8, "src")
    if src.dim() != 4 or src.shape[3] != 3:
        raise ValueError(f"src: expected [n_src, Hs, Ws, 3], got {tuple(src.shape)}")
    n_src, Hs, Ws = (int(v) for v in src.shape[:3])
    n = len(sel)
    if size is None:
        Ho, Wo = Hs, Ws
    else:
        Ho, Wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if min(n_src, Hs, Ws, n, Ho, Wo) < 1:
        raise ValueError(f"n_src, Hs, Ws, n, Ho, Wo must be positive, got {(n_src, Hs, Ws, n, Ho, Wo)}")
    if max(Hs, Ws, Ho, Wo) > MAX_SIZE or n > MAX_IMAGES:
        raise ValueError(f"images of up to {MAX_SIZE} pixels a side and up to {MAX_IMAGES} of them are supported, got "
                         f"{(Hs, Ws, Ho, Wo)} and {n}")
    sel = _table(sel, torch.int32, (n,), "sel", src)
    geom = None if geom is None else _table(geom, torch.int32, (n, 4), "geom", src)
    color = None if color is None else _table(color, torch.float32, (n, 4), "color", src)
    out = torch.empty((n, 3, Ho, Wo), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        rc = _hip.load().fpsg_episode_views(_hip.ptr(src), n_src, Hs, Ws, _hip.ptr(sel), n,
                                            None if geom is None else _hip.ptr(geom),
                                            None if color is None else _hip.ptr(color), _hip.ptr(out), Ho, Wo,
                                            _hip.stream_of(src))
    _hip.check(rc, "fpsg_episode_views")
    return out


def decode_episode(sample: dict) -> dict:
    """The uint8 image tensors of an uploaded episode (``xs``, ``xq``, ``xad``: ``[..., n, S, S, 3]``) replaced by their
    float batches ``[..., n, 3, S, S]``, one K30 launch each on the current stream, and the tables that came with them
    (``<key>_geom``, ``<key>_color``) taken out: what is left is the sample dict of the default datasets.  A sample whose
    images are floats already is returned as it is."""
    for key in IMAGE_KEYS:
        x = sample.get(key)
        geom, color = sample.pop(f"{key}_geom", None), sample.pop(f"{key}_color", None)
        if not torch.is_tensor(x) or x.dtype != torch.uint8:
            continue
        lead, (H, W, C) = tuple(x.shape[:-3]), x.shape[-3:]
        src = x.reshape(-1, H, W, C)
        n = src.shape[0]
        out = decode(src, torch.arange(n, dtype=torch.int32, device=src.device),
                     None if geom is None else geom.reshape(n, 4), None if color is None else color.reshape(n, 4))
        sample[key] = out.view(lead + (3, H, W))
    return sample


# ------------------------------------------------------------------------------------- draws
def draw(generator: torch.Generator, counts, S: int, geom_jitter: float = 0.0, color_jitter: float = 0.0):
    """An episode's per-image tables, drawn on the host from ``generator`` (never the global one): ``(view [n] int64,
    geom [n,4] int32, color [n,4] float32 or None)`` for images of ``S x S`` pixels whose items have ``counts [n]`` views.

    One ``torch.rand(n, 7, dtype=float64)`` call, whatever the jitters (the stream does not depend on them), columns
    ``u0 .. u6``, everything below in float64:
      * view ``= min(floor(u0 * count), count - 1)``;
      * zoom ``z = 1 - J + 2 J u1``; centre ``c = (S - 1) / 2 + S (J u - J / 2)`` with ``u2`` for x and ``u3`` for y;
        ``step = rint(256 z)``; ``x0 = rint(256 c - (S - 1) step / 2)`` (``J = 0``: the identity ``(0, 0, 256)``);
      * contrast ``= 1 - C + 2 C u4``, saturation ``= 1 - C + 2 C u5``, brightness ``= C (u6 - 1/2) / 2``, rounded to
        float32 at the end; ``C = 0``: no colour table at all."""
    counts = torch.as_tensor(counts, dtype=torch.float64).reshape(-1)
    J, C = float(geom_jitter), float(color_jitter)
    u = torch.rand(counts.numel(), 7, dtype=torch.float64, generator=generator)
    view = torch.minimum(torch.floor(u[:, 0] * counts), counts - 1).to(torch.int64)
    step = torch.round(256.0 * (1.0 - J + 2.0 * J * u[:, 1]))          # torch.round: half to even, as rint
    geom = torch.zeros(counts.numel(), 4, dtype=torch.int32)
    for axis in (0, 1):
        centre = (S - 1) / 2.0 + S * (J * u[:, 2 + axis] - J / 2.0)
        geom[:, axis] = torch.round(256.0 * centre - (S - 1) * step / 2.0).to(torch.int32)
    geom[:, 2] = step.to(torch.int32)
    color = None
    if C > 0.0:
        color = torch.zeros(counts.numel(), 4, dtype=torch.float32)
        color[:, 0] = (C * (u[:, 6] - 0.5) / 2.0).to(torch.float32)
        color[:, 1] = (1.0 - C + 2.0 * C * u[:, 4]).to(torch.float32)
        color[:, 2] = (1.0 - C + 2.0 * C * u[:, 5]).to(torch.float32)
    return view, geom, color


# ------------------------------------------------------------------------------------- corpora
class ViewCorpus:
    """Up to ``V`` views of every item as uint8 pixels: ``images [items, V, S, S, 3]`` (HWC, as PIL gives them; the slots
    past an item's count are zero and never drawn) and ``counts [items]`` int32.  ``corpus[...]`` indexes ``images``."""

    def __init__(self, images: torch.Tensor, counts: torch.Tensor):
        assert images.dtype == torch.uint8 and images.dim() == 5 and counts.shape == (images.shape[0],)
        self.images, self.counts = images, counts

    @classmethod
    def from_paths(cls, view_paths, transform, n_views: int = 0) -> "ViewCorpus":
        """``view_paths``: per item the image files, view 0 first.  ``n_views``: the slots per item, 0 = the longest
        list.  Every image goes through ``transform.to_uint8``: the crop and resize of the default pipeline."""
        V = n_views if n_views > 0 else max((len(p) for p in view_paths), default=1)
        S = transform.size
        images = torch.zeros((len(view_paths), V, S, S, 3), dtype=torch.uint8)
        counts = torch.zeros(len(view_paths), dtype=torch.int32)
        for i, paths in enumerate(view_paths):
            for v, path in enumerate(paths[:V]):
                images[i, v] = torch.from_numpy(transform.to_uint8(Image.open(path).convert("RGB")))
            counts[i] = min(len(paths), V)
        return cls(images, counts)

    V = property(lambda self: self.images.shape[1])

    def __len__(self):
        return self.images.shape[0]

    def __getitem__(self, index):
        return self.images[index]

    def rows(self) -> torch.Tensor:
        """``[items * V, S, S, 3]``: view ``v`` of item ``i`` is row ``i * V + v`` (no copy)."""
        return self.images.view((-1,) + tuple(self.images.shape[2:]))

    def narrow(self, start: int, length: int) -> "ViewCorpus":
        """Items ``start .. start + length - 1`` (no copy)."""
        return ViewCorpus(self.images.narrow(0, start, length), self.counts.narrow(0, start, length))

    def to(self, device) -> "ViewCorpus":
        return ViewCorpus(self.images.to(device), self.counts.to(device))


def modelnet_views(image_path: str) -> list:
    """The views of a ModelNet item: the list line's image first (what the default pipeline reads), then the other files
    of its directory in sorted order."""
    folder = os.path.dirname(image_path)
    rest = [os.path.join(folder, v) for v in sorted(os.listdir(folder))]
    return [image_path] + [p for p in rest if os.path.abspath(p) != os.path.abspath(image_path)]


# ------------------------------------------------------------------------------------- datasets
class _MultiView:
    """The multi-view form of a ``datasets._FewShotFiles`` class (mixed in front of it): the same lists, clouds and
    episode indices; images as ``ViewCorpus`` rows with a view, a window and a colour triple drawn per image."""

    def __init__(self, *args, n_views: int = 0, view_jitter: float = 0.0, view_color_jitter: float = 0.0, **kwargs):
        check_view_options(n_views, view_jitter, view_color_jitter)
        self.n_views, self.view_jitter, self.view_color_jitter = n_views, view_jitter, view_color_jitter
        self._views_rng = torch.Generator().manual_seed(0)
        super().__init__(*args, **kwargs)

    def seed_views(self, seed: int) -> None:
        """Reseeds the generator of the views, windows and colours (``trainNetwork.py``: once per epoch and rank)."""
        self._views_rng.manual_seed(int(seed))

    def _item_views(self, sub, index) -> list:
        raise NotImplementedError

    def _build_reference(self):
        assert self.auxiliary_dir is not None, "Auxiliary folder is not generated yet!!!"
        names, sizes, paths, pcs = [], [], [], []
        for name in sorted(os.listdir(self.auxiliary_dir)):
            if not name.endswith(".txt"):
                continue
            class_name = name.split(".")[0].split("+")[1]
            print(f"Building Reference dataset for {class_name} ...")
            # the default class's lists and clouds, item by item (same reads, same numpy draws), without its image read
            sub = type(self).sub_dataset(os.path.join(self.auxiliary_dir, name), transform=None,
                                         tgt_transform=self.tgt_tfs)
            paths += [self._item_views(sub, i) for i in range(len(sub))]
            pcs.append(torch.stack([torch.from_numpy(np.ascontiguousarray(self._item_cloud(sub, i), dtype=np.float32))
                                    for i in range(len(sub))]))
            names.append(class_name)
            sizes.append(len(sub))
        # one allocation for all classes: a class's corpus is a slice of it
        self.view_corpus = ViewCorpus.from_paths(paths, self.tfs, self.n_views)
        self.pc_corpus = torch.cat(pcs, dim=0)
        start = 0
        for class_name, size, pc in zip(names, sizes, pcs):
            self.reference[class_name] = {"views": self.view_corpus.narrow(start, size), "pcs": pc}
            start += size

    def _item_cloud(self, sub, index) -> np.ndarray:
        raise NotImplementedError

    def to(self, device):
        self.view_corpus = self.view_corpus.to(device)
        self.pc_corpus = self.pc_corpus.to(device)
        start = 0
        for entry in self.reference.values():
            size = len(entry["views"])
            entry["views"], entry["pcs"] = self.view_corpus.narrow(start, size), entry["pcs"].to(device)
            start += size
        return self

    def _images(self, corpus: ViewCorpus, idx: torch.Tensor, key: str, ans: dict) -> None:
        counts = corpus.counts.index_select(0, idx.to(corpus.counts.device)).cpu()
        view, geom, color = draw(self._views_rng, counts, corpus.images.shape[2], self.view_jitter,
                                 self.view_color_jitter)
        ans[key] = take_rows(corpus.rows(), idx * corpus.V + view)
        ans[f"{key}_geom"] = geom
        if color is not None:
            ans[f"{key}_color"] = color

    def __getitem__(self, index):
        key, shown = self.class_of(self.data_corpus[int(index)])
        entry = self.reference[key]
        n_query = self.n_query if self.n_query != -1 else len(entry["views"]) - self.n_support
        # the global stream: extract_episode's permutation, then the "ad" one, as in the default datasets
        example_idx = torch.randperm(len(entry["views"]))[:(self.n_support + n_query)]
        support_idx, query_idx = example_idx[:self.n_support], example_idx[self.n_support:]
        ad = torch.randperm(len(self.view_corpus))[:self.n_support]
        ans = {"class": shown}
        self._images(entry["views"], support_idx, "xs", ans)
        self._images(entry["views"], query_idx, "xq", ans)
        ans["pcs"] = take_rows(entry["pcs"], support_idx)
        ans["pcq"] = take_rows(entry["pcs"], query_idx)
        ans["tmp"] = int(query_idx[0]) if query_idx.numel() else -1
        self._images(self.view_corpus, ad, "xad", ans)
        ans["pcad"] = take_rows(self.pc_corpus, ad)
        return ans


class MultiViewModelNet(_MultiView, FewShotModelNet):
    def _item_views(self, sub, index):
        return modelnet_views(sub.imgs[index])

    def _item_cloud(self, sub, index):
        return to_unit_ball(np.asarray(sub.loader(sub.pcs[index]), dtype=np.float32), sub.n_pts)


class MultiViewShapeNet(_MultiView, FewShotShapeNet):
    def _item_views(self, sub, index):
        return sub.imgs[index]                      # sorted(os.listdir(images)), as the default class lists them

    def _item_cloud(self, sub, index):
        return to_unit_ball(sub.pc_data[index], sub.n_pts)
