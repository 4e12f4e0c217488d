"""The evaluation report's column table (``fpsg_amd/eval_report.py``), what needs no GPU: the parser built from the table
is the one the entry point has always had, the columns turn hand-made per-item results into the documented line and
return value in the two documented orders, and the ``*_from_rows`` forms of ``metrics`` refuse what ``fscore`` / ``dcd``
refuse before any device call."""
import statistics

import pytest
import torch

# (option strings, default, nargs, const, metavar, help) of every evaluation-only option besides --npy_folder, recorded
# from the parser as it was before the table existed (commit ccdeb2a), in the order --help lists them
RECORDED = [
    (['--exact_emd'], False, 0, True, None,
     'Also report the exact EMD per class (HIP auction, fpsg_amd.metrics.emd_exact);'),
    (['--set_metrics'], False, 0, True, None,
     'Also report MMD-CD, COV-CD and 1-NNA-CD per class over all its generated and reference query clouds (HIP Chamfer '
     'matrix, fpsg_amd.set_metrics);'),
    (['--set_metrics_emd'], False, 0, True, None,
     'Also report MMD-EMD, COV-EMD and 1-NNA-EMD per class over all its generated and reference query clouds (HIP exact '
     'EMD matrix, fpsg_amd.set_metrics);'),
    (['--set_metrics_points'], None, None, None, 'N',
     'With --set_metrics / --set_metrics_emd: reduce every generated and reference query cloud to N points by farthest '
     'point sampling from index 0 (HIP, fpsg_amd.sampling) before the set metrics; the labels become MMD-CD@N, ...; every '
     'other column stays on the full clouds;'),
    (['--jsd'], False, 0, True, None,
     'Also report the Jensen-Shannon divergence per class between the voxel-occupancy distributions of its generated and '
     'reference query clouds (HIP occupancy grid, fpsg_amd.set_metrics.jsd);'),
    (['--fscore'], None, '+', None, 'TAU',
     "Also report per class the F-score of the reconstructions at these distances (1 to 16 of them; share of points "
     "within TAU of the other cloud, precision and recall combined) and the Hausdorff distance (HIP distance profile, "
     "fpsg_amd.metrics.fscore); TAU is a Euclidean distance in the clouds' units: the clouds are normalised into the unit "
     "ball, so 0.02 is 1 %% of its diameter;"),
    (['--dcd'], None, '?', 1000.0, 'ALPHA',
     'Also report per class the density-aware Chamfer distance of the reconstructions (in [0, 1]; HIP, '
     'fpsg_amd.metrics.dcd); ALPHA is the factor on the squared distance [default: 1000];'),
]

ALL_LABELS = ["Rec CD", "Rec EMD", "Exact EMD", "F@0.02", "F@0.05", "HD", "DCD", "MMD-CD", "COV-CD", "1-NNA-CD", "MMD-EMD",
              "COV-EMD", "1-NNA-EMD", "EMD-uncertified", "JSD"]
ALL_FLAGS = ["--exact_emd", "--fscore", "0.02", "0.05", "--dcd", "--set_metrics", "--set_metrics_emd", "--jsd"]


def test_the_parser_built_from_the_table_is_the_recorded_one():
    from fpsg_amd import cli
    training = cli.few_shot_parser()
    shared = {a.dest for a in training._actions} | {"npy_folder"}
    got = [(a.option_strings, a.default, a.nargs, a.const, a.metavar, a.help)
           for a in cli.few_shot_parser(evaluation=True)._actions if a.dest not in shared]
    assert got == RECORDED
    strings = {s for a in training._actions for s in a.option_strings}
    assert not strings & {r[0][0] for r in RECORDED}, "the training parser has none of the report's options"
    assert "--dcd_alpha" in strings


def test_importing_the_table_loads_no_library(monkeypatch):
    import importlib

    from fpsg_amd import _hip
    monkeypatch.setattr(_hip, "load", lambda: pytest.fail("the HIP library was asked for"))
    from fpsg_amd import eval_report
    importlib.reload(eval_report)
    assert isinstance(eval_report.COLUMNS, tuple) and isinstance(eval_report.RETURN_ORDER, tuple)
    assert set(eval_report.COLUMNS) == set(eval_report.RETURN_ORDER) and len(eval_report.COLUMNS) == 6


# ---- hand-made items through the columns ---------------------------------------------------------------------------

def _items():
    """Two classes with two items each, as ``EvalItem`` with every keyword returns them (Q = 2, 8 points, T = 2)."""
    g = torch.Generator().manual_seed(5)
    out = {}
    for name in ("chair", "lamp"):
        out[name] = [{"cd_loss": torch.rand((), generator=g), "emd_loss": torch.rand((), generator=g),
                      "exact_emd": torch.rand((), generator=g),
                      "fscore": torch.rand(2, generator=g, dtype=torch.float64),
                      "precision": torch.rand(2, generator=g, dtype=torch.float64),
                      "recall": torch.rand(2, generator=g, dtype=torch.float64),
                      "hausdorff": torch.rand((), generator=g, dtype=torch.float64),
                      "dcd": torch.rand((), generator=g),
                      "syn_pc": torch.rand((2, 8, 3), generator=g), "ref_pc_q": torch.rand((2, 8, 3), generator=g)}
                     for _ in range(2)]
    return out


@pytest.fixture
def stubs(monkeypatch):
    """The device parts of the set-level columns, replaced by functions of the clouds' shapes and sums."""
    from fpsg_amd import metrics, sampling, set_metrics
    seen = {"subsample": [], "sets": []}

    def subsample(points, n, start=None):
        seen["subsample"].append((tuple(points.shape), n, start))
        return points[:, :n].contiguous()

    def gen_cd(gen, ref):
        seen["sets"].append(("cd", tuple(gen.shape), tuple(ref.shape)))
        return {"mmd_cd": float(gen.sum()), "cov_cd": 0.5, "nna_cd": float(ref.sum())}

    def gen_emd(gen, ref):
        seen["sets"].append(("emd", tuple(gen.shape), tuple(ref.shape)))
        return {"mmd_emd": float(gen.sum()) + 1.0, "cov_emd": 0.75, "nna_emd": 0.625, "mmd_emd_lower": 0.0,
                "cov_uncertified": 0.25, "nna_uncertified": 0.0}

    def grid(clouds, out=None):
        return {"n": clouds.size(0) + (0 if out is None else out["n"])}

    monkeypatch.setattr(sampling, "farthest_point_subsample", subsample)
    monkeypatch.setattr(set_metrics, "generation_metrics", gen_cd)
    monkeypatch.setattr(set_metrics, "emd_generation_metrics", gen_emd)
    monkeypatch.setattr(metrics, "occupancy_grid", grid)
    monkeypatch.setattr(set_metrics, "jsd_from_grids", lambda g, r: {"jsd": 1.0 / (g["n"] + r["n"])})
    return seen


def _report(argv, items, n_query=2):
    """What ``evaluate_Network.main`` does with the items of its loop: ``(lines, returned tuple)``."""
    from fpsg_amd import cli, eval_report
    opt = cli.few_shot_parser(evaluation=True).parse_args(["--synthetic", "--n_way", "1"] + argv)
    cli.validate(opt)
    columns = eval_report.active_columns(opt)
    cd, emd = {}, {}
    for name, outs in items.items():
        for out in outs:
            out = dict(out)
            cd.setdefault(name, []).append(out["cd_loss"].item() / n_query)
            emd.setdefault(name, []).append(out["emd_loss"].item() / n_query)
            for column in columns:
                column.add(name, out, n_query)
    for column in columns:
        column.finish()
    lines = [eval_report.line(n, statistics.mean(cd[n]), statistics.mean(emd[n]), columns) for n in sorted(cd)]
    return lines, (cd, emd) + eval_report.results(columns), columns


def _fields(line):
    head, body = line.split(" -- ")
    return head[len("Class: "):], [tuple(f.split(": ")) for f in body.split("; ")]


def test_every_flag_the_line_and_the_returned_values(stubs):
    items = _items()
    lines, res, _ = _report(ALL_FLAGS, items)
    assert len(lines) == 2 and len(res) == 8
    cd, emd, exact, set_cd, set_emd, jsd, f, dcd = res                 # the return order
    assert stubs["sets"] == [("cd", (4, 8, 3), (4, 8, 3))] * 2 + [("emd", (4, 8, 3), (4, 8, 3))] * 2
    assert not stubs["subsample"]
    for line in lines:
        name, fields = _fields(line)
        assert line.startswith("Class: ") and [label for label, _ in fields] == ALL_LABELS, line
        outs = items[name]
        # the returned objects, from the items by hand
        assert exact[name] == [o["exact_emd"].item() / 2 for o in outs] and type(exact).__name__ == "defaultdict"
        assert dcd[name] == [o["dcd"].item() for o in outs] and type(dcd).__name__ == "defaultdict"
        assert set(f[name]) == {"thresholds", "fscore", "precision", "recall", "hausdorff"}
        assert f[name]["thresholds"] == [0.02, 0.05]
        for key in ("fscore", "precision", "recall"):
            assert f[name][key] == [statistics.mean(o[key][t].item() for o in outs) for t in range(2)]
            assert all(type(v) is float for v in f[name][key])
        assert f[name]["hausdorff"] == statistics.mean(o["hausdorff"].item() for o in outs)
        gen, ref = torch.cat([o["syn_pc"] for o in outs]), torch.cat([o["ref_pc_q"] for o in outs])
        assert set_cd[name] == {"mmd_cd": float(gen.sum()), "cov_cd": 0.5, "nna_cd": float(ref.sum())}
        assert set_emd[name]["mmd_emd"] == float(gen.sum()) + 1.0 and set_emd[name]["cov_uncertified"] == 0.25
        assert jsd[name] == {"jsd": 1.0 / 8}
        # every value printed is str() of the returned one
        want = [statistics.mean(cd[name]), statistics.mean(emd[name]), statistics.mean(exact[name]), *f[name]["fscore"],
                f[name]["hausdorff"], statistics.mean(dcd[name]), set_cd[name]["mmd_cd"], set_cd[name]["cov_cd"],
                set_cd[name]["nna_cd"], set_emd[name]["mmd_emd"], set_emd[name]["cov_emd"], set_emd[name]["nna_emd"],
                f"{set_emd[name]['cov_uncertified']}/{set_emd[name]['nna_uncertified']}", jsd[name]["jsd"]]
        assert [text for _, text in fields] == [str(v) for v in want], line


def test_the_line_order_does_not_depend_on_the_order_of_the_flags(stubs):
    lines, _, _ = _report(ALL_FLAGS, _items())
    again, _, _ = _report(["--jsd", "--set_metrics_emd", "--set_metrics", "--dcd", "1000", "--fscore", "0.02", "0.05",
                           "--exact_emd"], _items())
    assert again == lines


def test_certified_set_metrics_print_no_uncertified_field(stubs, monkeypatch):
    from fpsg_amd import set_metrics
    inner = set_metrics.emd_generation_metrics
    monkeypatch.setattr(set_metrics, "emd_generation_metrics",
                        lambda g, r: dict(inner(g, r), cov_uncertified=0.0, nna_uncertified=0.0))
    lines, _, _ = _report(ALL_FLAGS, _items())
    for line in lines:
        assert [label for label, _ in _fields(line)[1]] == [lb for lb in ALL_LABELS if lb != "EMD-uncertified"]


def test_reduced_set_metrics_mark_their_six_labels_only(stubs):
    items = _items()
    lines, res, _ = _report(ALL_FLAGS + ["--set_metrics_points", "4"], items)
    # both clouds of every item reduced once, whichever of the two groups reads them; only reduced clouds are kept
    assert stubs["subsample"] == [((2, 8, 3), 4, 0)] * 8
    assert stubs["sets"] == [("cd", (4, 4, 3), (4, 4, 3))] * 2 + [("emd", (4, 4, 3), (4, 4, 3))] * 2
    marked = {"MMD-CD", "COV-CD", "1-NNA-CD", "MMD-EMD", "COV-EMD", "1-NNA-EMD"}
    for line in lines:
        labels = [label for label, _ in _fields(line)[1]]
        assert labels == [lb + "@4" if lb in marked else lb for lb in ALL_LABELS], line
    big = {n: [dict(o, syn_pc=torch.zeros(2, 600, 3), ref_pc_q=torch.zeros(2, 600, 3)) for o in outs]
           for n, outs in items.items()}
    lines, _, _ = _report(ALL_FLAGS + ["--set_metrics_points", "512"], big)
    for line in lines:
        labels = [label for label, _ in _fields(line)[1]]
        assert labels == [lb + "@512" if lb in marked else lb for lb in ALL_LABELS], line
    with pytest.raises(ValueError, match=r"--set_metrics_points 512 exceeds the 8 points of the generated clouds"):
        _report(["--set_metrics_emd", "--set_metrics_points", "512"], items)


@pytest.mark.parametrize("flag, position", [(["--exact_emd"], 2), (["--set_metrics"], 3), (["--set_metrics_emd"], 4),
                                            (["--jsd"], 5), (["--fscore", "0.02", "0.05"], 6), (["--dcd"], 7)])
def test_each_flag_alone_adds_its_one_element(stubs, flag, position):
    full = _report(ALL_FLAGS, _items())[1]
    lines, res, columns = _report(flag, _items())
    assert len(res) == 3 and len(columns) == 1
    assert res[:2] == full[:2] and res[2] == full[position] and type(res[2]) is type(full[position])
    plain = _report([], _items())
    assert len(plain[1]) == 2 and all(ln.startswith(pl + "; ") for pl, ln in zip(plain[0], lines))


def test_threshold_labels_are_the_repr_of_the_float_as_given(stubs):
    items = {n: [dict(o, fscore=o["fscore"].repeat(2)[:3], precision=o["precision"].repeat(2)[:3],
                      recall=o["recall"].repeat(2)[:3]) for o in outs] for n, outs in _items().items()}
    lines, res, _ = _report(["--fscore", "0.1", "1e-3", "2"], items)
    for line in lines:
        assert [label for label, _ in _fields(line)[1]] == ["Rec CD", "Rec EMD", "F@0.1", "F@0.001", "F@2.0", "HD"]
    assert all(m["thresholds"] == [0.1, 0.001, 2.0] for m in res[2].values())


def test_item_options_and_item_columns():
    """What ``main`` opens ``EvalItem`` with, and the per-item parts ``EvalItem`` makes of its keywords."""
    from fpsg_amd import cli, eval_report
    parser = cli.few_shot_parser(evaluation=True)

    def options(argv):
        return eval_report.item_options(eval_report.active_columns(parser.parse_args(argv)))

    assert options([]) == {}
    assert options(["--exact_emd"]) == {"exact_emd": True}
    assert options(["--fscore", "0.02", "0.05"]) == {"fscore": (0.02, 0.05)}
    assert options(["--dcd"]) == {"dcd": 1000.0} and options(["--dcd", "40"]) == {"dcd": 40.0}
    for flag in ("--set_metrics", "--set_metrics_emd", "--jsd"):
        assert options([flag]) == {"return_clouds": True}
    assert options(ALL_FLAGS) == {"exact_emd": True, "fscore": (0.02, 0.05), "dcd": 1000.0, "return_clouds": True}
    assert eval_report.item_columns() == []
    cols = eval_report.item_columns(exact_emd=True, fscore=[0.02], dcd=0)
    assert [type(c) for c in cols] == [eval_report.ExactEmd, eval_report.FScore, eval_report.Dcd]
    assert [c.needs_rows for c in cols] == [False, True, True]
    assert cols[1].thresholds == (0.02,) and cols[2].alpha == 0.0
    with pytest.raises(ValueError):
        eval_report.item_columns(fscore=[-1.0])
    with pytest.raises(ValueError):
        eval_report.item_columns(dcd=float("nan"))


# ---- the *_from_rows forms refuse what fscore / dcd refuse, before any device call ---------------------------------

def _rows(B=2, N=8, M=6):
    return (torch.zeros(B, N), torch.zeros(B, M), torch.zeros(B, N, dtype=torch.int32),
            torch.zeros(B, M, dtype=torch.int32))


def test_from_rows_forms_check_before_any_device_call(monkeypatch):
    from fpsg_amd import _hip
    from fpsg_amd.metrics import DCD_MAX_N, dcd, dcd_from_rows, fscore, fscore_from_rows
    monkeypatch.setattr(_hip, "load", lambda: pytest.fail("the HIP library was asked for"))
    rows = _rows()
    clouds = torch.zeros(2, 8, 3), torch.zeros(2, 6, 3)
    for bad in ([], [0.1] * 17, [-0.01], [float("inf")], "0.02", 0.02, [None]):
        for call in (lambda: fscore_from_rows(rows, bad), lambda: fscore(*clouds, bad)):
            with pytest.raises(ValueError, match="thresholds"):
                call()
    with pytest.raises(ValueError, match="thresholds"):               # thresholds first, then the rows
        fscore_from_rows((torch.zeros(2), torch.zeros(2, 6)), [-1.0])
    for d1, d2, what in ((torch.zeros(8), rows[1], "dist1"), (rows[0], torch.zeros(2, 6, 1), "dist2"),
                         (rows[0], torch.zeros(3, 6), "batch mismatch"), (rows[0], torch.zeros(2, 0), "empty")):
        with pytest.raises(ValueError, match=what):
            fscore_from_rows((d1, d2, None, None), [0.02])
    for bad in (-1.0, float("nan"), float("inf"), "x", None):
        for call in (lambda: dcd_from_rows(rows, bad), lambda: dcd(*clouds, bad)):
            with pytest.raises(ValueError, match="alpha"):
                call()
    with pytest.raises(ValueError, match="alpha"):                    # alpha first, then the rows
        dcd_from_rows((torch.zeros(2),) * 4, -1.0)
    d1, d2, i1, i2 = rows
    for bad, what in (((torch.zeros(8), d2, i1, i2), "K1's rows"), ((d1, d2, i2, i1), "K1's rows"),
                      ((d1, d2, i1, None), "K1's rows"), (_rows(2, 8, 6)[:1] + _rows(3, 8, 6)[1:2] + (i1, torch.zeros(
                          3, 6, dtype=torch.int32)), "batch mismatch"),
                      (_rows(2, 8, 0), "empty"), (_rows(1, DCD_MAX_N + 1, 3), f"at most {DCD_MAX_N}")):
        with pytest.raises(ValueError, match=what):
            dcd_from_rows(bad, 1000.0)
    with pytest.raises(ValueError, match=f"at most {DCD_MAX_N}"):
        dcd(torch.zeros(1, DCD_MAX_N + 1, 3), torch.zeros(1, 3, 3))
    # CPU rows that pass every check: no CPU path, as for the clouds
    with pytest.raises(_hip.FpsgHipError):
        dcd_from_rows(rows, 1000.0)
    with pytest.raises(_hip.FpsgHipError):
        fscore_from_rows(rows, [0.02])
