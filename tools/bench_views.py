"""K30 alone and in the episode's data path.  In one process, alternating over --rounds rounds after a warm-up:
  (a) the default form: a host-resident float32 corpus of 512 synthetic images, take_rows of 69 rows (a 32-shot episode's
      images) into the pinned ring, upload -- milliseconds per episode by a host clock around a synchronised window;
  (b) the multi-view form: a uint8 corpus of 512 x 12 views, take_rows, upload, one K30 launch over the 69 images with a
      window and a colour triple per image;
  (c) K30 alone by device events at 69 images of 224 x 224, with null tables and with both tables, in microseconds and as
      a share of the HBM bound on its compulsory bytes (one read of the uint8 images, one write of the floats).
Appends its figures to profiles/k30/views_notes.txt.

    python tools/bench_views.py [--items 512] [--views 12] [--n 69] [--rounds 3] [--episodes 40] [--iters 200]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from fpsg_amd import _hip, cli, episodes, views

NOTES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "k30", "views_notes.txt")
HBM_PEAK = 8.0e12           # bytes/s, the MI355X's HBM3E peak (spec)
S = 224


def episode_loop(corpus, draw, finish, n_episodes, ring, stream, dev):
    """``n_episodes`` times: draw row indices, gather them into the ring's pinned buffers, upload on ``stream``, ``finish``
    on it.  -> milliseconds per episode."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_episodes):
        ring.next_episode()
        rows, tables = draw()
        host = episodes.take_rows(corpus, rows)
        with torch.cuda.stream(stream):
            x = host.to(dev, non_blocking=True)
            finish(x, tables)
            event = torch.cuda.Event()
            event.record(stream)
        ring.uploaded(event)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n_episodes * 1e3


def data_path(a, out):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    floats = episodes.synthetic_images(a.items, S, g)                                    # [items, 3, S, S] float32
    pixels = torch.randint(0, 256, (a.items * a.views, S, S, 3), dtype=torch.uint8, generator=g)
    counts = torch.full((a.n,), a.views)
    ring = episodes._staging.ring = episodes._PinnedRing(4)
    stream = torch.cuda.Stream(device=dev)

    def draw_default():
        return torch.randperm(a.items, generator=g)[:a.n], None

    def draw_views():
        view, geom, color = views.draw(g, counts, S, 0.2, 0.4)
        return torch.randperm(a.items, generator=g)[:a.n] * a.views + view, (geom, color)

    def decode(x, tables):
        views.decode(x, torch.arange(a.n, dtype=torch.int32, device=dev), *tables)

    forms = {"(a) float32 corpus: take_rows + upload": (floats, draw_default, lambda x, tables: None),
             "(b) uint8 corpus: take_rows + upload + K30, both jitters": (pixels, draw_views, decode)}
    times = {name: [] for name in forms}
    for name, (corpus, draw, finish) in forms.items():
        episode_loop(corpus, draw, finish, 8, ring, stream, dev)                          # warm-up: the ring's buffers
    for _ in range(a.rounds):
        for name, (corpus, draw, finish) in forms.items():
            times[name].append(episode_loop(corpus, draw, finish, a.episodes, ring, stream, dev))
    episodes._staging.ring = None
    mb = {name: a.n * corpus[0].numel() * corpus.element_size() / 1e6 for name, (corpus, _, _) in forms.items()}
    for name, ts in times.items():
        out.append(f"{name:>58}: {min(ts):7.2f} - {max(ts):7.2f} ms per episode over {a.rounds} alternating rounds of "
                   f"{a.episodes} ({a.n} images, {mb[name]:.1f} MB uploaded; corpus of {a.items} items"
                   f"{' x %d views' % a.views if 'uint8' in name else ''}, {cli.usable_cores()} host threads)")


def timed(fn, iters):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us


def kernel(a, out):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    src = torch.randint(0, 256, (a.n, S, S, 3), dtype=torch.uint8, generator=g).to(dev)
    sel = torch.randperm(a.n, generator=g).to(torch.int32).to(dev)
    _, geom, color = views.draw(g, torch.full((a.n,), a.views), S, 0.2, 0.4)
    geom, color = geom.to(dev), color.to(dev)
    out_t = torch.empty((a.n, 3, S, S), dtype=torch.float32, device=dev)
    assert torch.equal(views.decode(src, sel, geom, color), views.decode(src, sel.cpu(), geom.cpu(), color.cpu()))
    lib, stream = _hip.load(), _hip.stream_of(src)

    def entry(geom_ptr, color_ptr):       # the entry itself into one output: the wrapper's allocation would pace the loop
        _hip.check(lib.fpsg_episode_views(src.data_ptr(), a.n, S, S, sel.data_ptr(), a.n, geom_ptr, color_ptr,
                                          out_t.data_ptr(), S, S, stream), "fpsg_episode_views")

    forms = {"K30, null tables": lambda: entry(None, None),
             "K30, window and colour per image": lambda: entry(geom.data_ptr(), color.data_ptr())}
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, fn in forms.items():
            times[name].append(timed(fn, a.iters))
    compulsory = a.n * (S * S * 3 + S * S * 3 * 4)     # one read of the uint8 images, one write of the floats
    bound = compulsory / HBM_PEAK * 1e6                # us: of the two roofline bounds the larger one (the arithmetic's is ~5.5 us)
    for name, ts in times.items():
        out.append(f"{name:>58}: {min(ts):7.1f} - {max(ts):7.1f} us per call (device events around {a.iters} "
                   f"back-to-back calls) over {a.rounds} rounds of {a.iters}; compulsory bytes {compulsory} = {a.n} x (150528 read + "
                   f"602112 written), HBM bound at 8.0 TB/s {bound:.1f} us: {100 * bound / max(ts):.0f} - "
                   f"{100 * bound / min(ts):.0f} % of the bandwidth bound")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=512)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--n", type=int, default=69)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--episodes", type=int, default=40)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    cli.limit_host_threads()
    out = [f"# tools/bench_views.py on {torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}"]
    kernel(a, out)
    data_path(a, out)
    print("\n".join(out))
    os.makedirs(os.path.dirname(NOTES), exist_ok=True)
    with open(NOTES, "a") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
