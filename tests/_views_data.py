"""Tiny ModelNet and ShapeNet trees with several views per item, for the multi-view tests (tests/test_views_*.py):
2 classes x 5 items x 3 views, one item with only 2 views; images of several sizes, one of them not square."""
import numpy as np
from PIL import Image

CLASSES = {"modelnet": ("cup", "door"), "shapenet": ("02880940", "03797390")}
ITEMS, VIEWS = 5, 3
SHORT = (1, 3)                      # (class, item) of the item with two views


def _image(rng, path, w, h):
    # smooth enough to compress, random enough that no two views agree
    small = rng.integers(0, 256, (h // 20 + 1, w // 20 + 1, 3), dtype=np.uint8)
    Image.fromarray(small).resize((w, h), Image.BILINEAR).save(path)


def _n_views(c, i):
    return VIEWS - 1 if (c, i) == SHORT else VIEWS


def _write_ply(path, pts):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "end_header\n" % len(pts))
        for p in pts:
            f.write("%f %f %f\n" % tuple(p))


def modelnet_tree(root, seed=0):
    """-> (config file, auxiliary dir).  The list line names view ``v1.png``: NOT the first file of its directory, so
    view 0 is the line's image and the others follow in sorted order."""
    rng = np.random.default_rng(seed)
    aux = root / "aux"
    aux.mkdir()
    lines = []
    for c, cls in enumerate(CLASSES["modelnet"]):
        cl = []
        for i in range(ITEMS):
            d = root / "img" / cls / "train" / f"{cls}_{i}"
            d.mkdir(parents=True)
            for v in range(_n_views(c, i)):
                _image(rng, d / f"v{v}.png", 600 if i else 580, 600 if i != 2 else 560)
            ply = root / f"{cls}_{i}.ply"
            _write_ply(ply, rng.standard_normal((40 + i, 3)) * 3 + 1)
            cl.append(f"{d / 'v1.png'}\t{ply}")
        (aux / f"modelnet+{cls}.txt").write_text("\n".join(cl))
        lines += cl
    cfg = root / "modelnet_train.txt"
    cfg.write_text("\n".join(lines))
    return str(cfg), str(aux)


def shapenet_tree(root, seed=1):
    rng = np.random.default_rng(seed)
    aux = root / "aux"
    aux.mkdir()
    lines = []
    for c, syn in enumerate(CLASSES["shapenet"]):
        cl = []
        for i in range(ITEMS):
            item = root / "ShapeNet" / syn / f"m{i}"
            (item / "images").mkdir(parents=True)
            for v in range(_n_views(c, i)):
                _image(rng, item / "images" / f"{v:02d}.png", 256 if i else 300, 256 if i != 2 else 200)
            np.save(item / "npy_file.npy", rng.standard_normal((15000, 3)).astype(np.float32))
            cl.append(str(item))
        (aux / f"shapenet+{syn}.txt").write_text("\n".join(cl))
        lines += cl
    cfg = root / "shapenet_train.txt"
    cfg.write_text("\n".join(lines))
    return str(cfg), str(aux)
