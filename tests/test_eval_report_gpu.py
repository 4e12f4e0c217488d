"""The evaluation report's columns on the GPU (``fpsg_amd/eval_report.py``): an item with every extra at once returns,
bit for bit, what an item with each extra alone returns; the columns that read K1's rows share one K1 forward; and
``evaluate_Network.py`` with every flag reports, element by element, what it reports with each flag alone."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

TAUS = (0.02, 0.05)
ALPHA = 1000.0
F_KEYS = ("fscore", "precision", "recall", "hausdorff")


@pytest.fixture(scope="module")
def model(gpu):
    from fpsg_amd.engine import build_model, default_options
    torch.manual_seed(3)
    return build_model(default_options(device="cuda")).to(gpu).eval()


def _fixed_grids(model, monkeypatch, Q, gpu):
    """The decoder's sampling grids drawn once, so that separate runs generate the same clouds."""
    grids = model.pc_decoder.sample_grids(Q, gpu, torch.Generator(device=gpu).manual_seed(9))
    orig = model.pc_decoder.forward
    monkeypatch.setattr(model.pc_decoder, "forward",
                        lambda h, grid=None, generator=None, pack=None: orig(h, grid=grids, pack=pack))


def _episodes(Q, gpu, n=4):
    from fpsg_amd.episodes import synthetic_episode
    return [synthetic_episode(1, Q, n_pts=2048, img_size=96, seed=80 + i, device=gpu) for i in range(n)]


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("Q", [1, 2])
def test_all_extras_at_once_equal_each_alone(gpu, model, monkeypatch, Q, graph):
    """Four items (two eager, the capture, one replay with the graph on): every key of the item with all extras equals
    the same key of the item that has only that extra, and the F-score / DCD fields equal the ``*_from_rows`` forms on
    ``nearest_rows`` of the returned clouds and ``metrics.fscore`` / ``metrics.dcd`` on them."""
    from fpsg_amd.engine import EvalItem
    from fpsg_amd.metrics import dcd, dcd_from_rows, fscore, fscore_from_rows, nearest_rows
    _fixed_grids(model, monkeypatch, Q, gpu)
    eps = _episodes(Q, gpu)

    def run(**extras):
        with EvalItem(model, graph=graph, **extras) as item:
            outs = [item(ep) for ep in eps]
            assert bool(item._graphs) == graph, "the third item of a shape is captured, with the graph on"
        return outs

    everything = run(exact_emd=True, fscore=TAUS, dcd=ALPHA, return_clouds=True)
    alone = {("cd_loss", "emd_loss"): run(), ("exact_emd",): run(exact_emd=True), F_KEYS: run(fscore=TAUS),
             ("dcd",): run(dcd=ALPHA), ("syn_pc", "ref_pc_q"): run(return_clouds=True)}
    base = {"cd_loss", "emd_loss"}
    for keys, outs in alone.items():
        for i, (a, e) in enumerate(zip(outs, everything)):
            assert set(a) == base | set(keys)
            for key in base | set(keys):
                assert a[key].dtype == e[key].dtype and torch.equal(a[key], e[key]), (keys, i, key)
    for e in everything:
        assert set(e) == base | {"exact_emd", "dcd", "syn_pc", "ref_pc_q"} | set(F_KEYS)
        gen, ref = e["syn_pc"].contiguous(), e["ref_pc_q"].contiguous()
        rows = nearest_rows(gen, ref)
        assert len(rows) == 4 and not any(r.requires_grad for r in rows)
        for want in (fscore_from_rows(rows, TAUS), fscore(gen, ref, TAUS)):
            assert tuple(want["fscore"].shape) == (Q, 2)
            for key in ("fscore", "precision", "recall"):
                assert e[key].dtype == torch.float64 and torch.equal(e[key], want[key].mean(dim=0)), key
            assert e["hausdorff"].dim() == 0 and torch.equal(e["hausdorff"], want["hausdorff"].mean())
        for want in (dcd_from_rows(rows, ALPHA), dcd(gen, ref, ALPHA)):
            assert tuple(want.shape) == (Q,) and want.dtype == torch.float32
            assert e["dcd"].dim() == 0 and torch.equal(e["dcd"], want.mean())


def test_k1_runs_once_for_both_columns(gpu, model):
    """Launches per item by kind, eager items with Q = 2: the Chamfer loss's K1 forward, and ONE more for the columns
    that read K1's rows, whether one of them is on or both.  Before the columns shared the rows (``metrics.fscore`` and
    ``metrics.dcd`` each ran K1's forward) the case with both gave 3: it is the one assertion here that the code before
    this table did not meet."""
    from fpsg_amd import metrics
    from fpsg_amd.engine import EvalItem
    eps = _episodes(2, gpu, n=2)
    counts = {}

    def probe(kind, B, N, M):
        counts[kind] = counts.get(kind, 0) + 1
        return contextlib.nullcontext()

    cases = (({}, 1, 0, 0), ({"fscore": TAUS}, 2, 1, 0), ({"dcd": ALPHA}, 2, 0, 1),
             ({"fscore": TAUS, "dcd": ALPHA}, 2, 1, 1))
    try:
        for extras, k1, k17, k18 in cases:
            with EvalItem(model, graph=False, **extras) as item:
                for ep in eps:
                    counts.clear()
                    metrics.set_launch_probe(probe)
                    item(ep)
                    metrics.set_launch_probe(None)
                    got = (counts.get("chamfer_fwd", 0), counts.get("dist_profile", 0), counts.get("dcd", 0))
                    assert got == (k1, k17, k18), (extras, got)
    finally:
        metrics.set_launch_probe(None)


LABELS = ["Rec CD", "Rec EMD", "Exact EMD", "F@0.02", "F@0.05", "HD", "DCD", "MMD-CD@256", "COV-CD@256", "1-NNA-CD@256",
          "MMD-EMD@256", "COV-EMD@256", "1-NNA-EMD@256", "EMD-uncertified", "JSD"]


def test_entry_point_with_every_flag_reports_what_each_flag_alone_reports(gpu, tmp_path, capsys):
    import evaluate_Network
    from fpsg_amd import cli
    argv = ["--synthetic", "--n_shot", "2", "--n_query", "2", "--sequential_eval", "--model_path", str(tmp_path),
            "--name", "x"]
    parser = cli.few_shot_parser(evaluation=True)

    def run(extra):
        torch.manual_seed(0)
        res = evaluate_Network.main(parser.parse_args(argv + extra))
        return res, [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Class: ")]

    points = ["--set_metrics_points", "256"]
    single = [["--exact_emd"], ["--set_metrics"] + points, ["--set_metrics_emd"] + points, ["--jsd"],
              ["--fscore", "0.02", "0.05"], ["--dcd"]]              # in the order of the returned tuple
    res, lines = run(["--exact_emd", "--fscore", "0.02", "0.05", "--dcd", "--set_metrics", "--set_metrics_emd"] + points
                     + ["--jsd"])
    res_plain, plain = run([])
    assert len(res) == 8 and len(res_plain) == 2 and plain and len(lines) == len(plain)
    assert res[0] == res_plain[0] and res[1] == res_plain[1]
    for k, flags in enumerate(single):
        res_one, _ = run(flags)
        assert len(res_one) == 3
        assert res_one[-1] == res[2 + k] and type(res_one[-1]) is type(res[2 + k]), flags
        assert set(res[2 + k]) == set(res[0]), flags
    set_emd = res[4]
    for pl, ln in zip(plain, lines):
        name = ln.split(" -- ")[0][len("Class: "):]
        m = set_emd[name]
        certified = not (m["cov_uncertified"] or m["nna_uncertified"])
        labels = [f.split(": ")[0] for f in ln.split(" -- ")[1].split("; ")]
        assert labels == [lb for lb in LABELS if not (certified and lb == "EMD-uncertified")], ln
        assert ln.partition("; Exact EMD")[0] == pl, (pl, ln)      # cut at the first extra: the plain line, every character
