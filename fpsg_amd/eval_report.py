"""The optional columns of the evaluation report (``evaluate_Network.py``), one class per column group.

A group owns everything that is specific to it: its command-line argument(s) and their check, the ``EvalItem`` keyword
that switches its per-item part on, what that part computes on the device after an item, how the host accumulates it per
class, what is finished after the loop, the ``(label, value)`` fields it adds to a class's line and the per-class object
it adds to ``main``'s return value.  ``cli.few_shot_parser(evaluation=True)``, ``cli.validate``, ``engine.EvalItem`` and
``evaluate_Network.main`` loop over the groups; none of them names a metric.  To add a metric: one class here, one entry
in ``COLUMNS`` and one in ``RETURN_ORDER``.

Importing this module loads no library and touches no device.
"""
from __future__ import annotations

import statistics
from collections import defaultdict

import torch

from . import metrics, sampling, set_metrics


class Column:
    """One column group.  ``from_options(opt)`` is the group as the command line asks for it, or None."""

    needs_rows = False              # the per-item part reads K1's rows (metrics.nearest_rows) of the item's clouds

    @staticmethod
    def add_arguments(group) -> None:
        raise NotImplementedError

    @staticmethod
    def check(opt) -> None:
        """``SystemExit`` for option values the group cannot take."""

    @classmethod
    def from_options(cls, opt):
        raise NotImplementedError

    def item_options(self) -> dict:
        """The ``EvalItem`` keywords the group needs: its own, or ``return_clouds``."""
        return {"return_clouds": True}

    def per_item(self, syn_pc, ref_pc_q, rows) -> dict:
        """``EvalItem``: the group's entries of an item's result, on the device, from the item's contiguous clouds."""
        raise NotImplementedError

    def add(self, name, out, n_query) -> None:
        """``main``: take one item's result ``out`` of class ``name``."""
        raise NotImplementedError

    def finish(self) -> None:
        """``main``, after the loop: what is left to compute for ``self.result``."""

    def fields(self, name) -> list:
        """``[(label, value), ...]`` of class ``name``'s line."""
        raise NotImplementedError


class ExactEmd(Column):
    """``--exact_emd``: the exact transport distance (K12) summed over an item's queries, divided by ``n_query`` like the
    two reference metrics and averaged over the class's items."""

    def __init__(self):
        self.result = defaultdict(list)

    @staticmethod
    def add_arguments(group):
        group.add_argument("--exact_emd", action="store_true",
                           help="Also report the exact EMD per class (HIP auction, fpsg_amd.metrics.emd_exact);")

    @classmethod
    def from_options(cls, opt):
        return cls() if getattr(opt, "exact_emd", False) else None

    def item_options(self):
        return {"exact_emd": True}

    def per_item(self, syn_pc, ref_pc_q, rows):
        return {"exact_emd": metrics.emd_exact(syn_pc, ref_pc_q).sum()}

    def add(self, name, out, n_query):
        self.result[name].append(out["exact_emd"].item() / n_query)

    def fields(self, name):
        return [("Exact EMD", statistics.mean(self.result[name]))]


class FScore(Column):
    """``--fscore TAU [TAU ...]``: F-score, precision and recall at every threshold and the Hausdorff distance (K17 over
    K1's minima), averaged over an item's queries on the device and then over the class's items."""

    needs_rows = True

    def __init__(self, thresholds):
        self.thresholds = metrics.check_thresholds(thresholds)
        self.items = defaultdict(list)      # per class and item: [fscore [T], precision [T], recall [T], hd]
        self.result = {}

    @staticmethod
    def add_arguments(group):
        group.add_argument("--fscore", type=float, nargs="+", default=None, metavar="TAU",
                           help="Also report per class the F-score of the reconstructions at these distances (1 to 16 of "
                                "them; share of points within TAU of the other cloud, precision and recall combined) and "
                                "the Hausdorff distance (HIP distance profile, fpsg_amd.metrics.fscore); TAU is a "
                                "Euclidean distance in the clouds' units: the clouds are normalised into the unit ball, "
                                "so 0.02 is 1 %% of its diameter;")

    @staticmethod
    def check(opt):
        taus = getattr(opt, "fscore", None)
        if taus is None:
            return
        if len(taus) > metrics.PROFILE_MAX_T:
            raise SystemExit(f"--fscore takes at most {metrics.PROFILE_MAX_T} thresholds (got {len(taus)})")
        try:
            metrics.check_thresholds(taus)
        except ValueError as e:
            raise SystemExit(f"--fscore: {e}") from None

    @classmethod
    def from_options(cls, opt):
        taus = getattr(opt, "fscore", None)
        return None if taus is None else cls(tuple(taus))

    def item_options(self):
        return {"fscore": self.thresholds}

    def per_item(self, syn_pc, ref_pc_q, rows):
        f = metrics.fscore_from_rows(rows, self.thresholds)
        out = {key: f[key].mean(dim=0) for key in ("fscore", "precision", "recall")}
        out["hausdorff"] = f["hausdorff"].mean()
        return out

    def add(self, name, out, n_query):      # the item's means over its queries, in one host read
        self.items[name].append(torch.stack([out["fscore"], out["precision"], out["recall"],
                                             out["hausdorff"].expand(len(self.thresholds))]).tolist())

    def finish(self):
        T = range(len(self.thresholds))
        for name in sorted(self.items):
            f, p, r, hd = ([[item[k][t] for item in self.items[name]] for t in T] for k in range(4))
            self.result[name] = {"thresholds": list(self.thresholds), "fscore": [statistics.mean(v) for v in f],
                                 "precision": [statistics.mean(v) for v in p],
                                 "recall": [statistics.mean(v) for v in r], "hausdorff": statistics.mean(hd[0])}

    def fields(self, name):
        m = self.result[name]
        return [(f"F@{tau!r}", v) for tau, v in zip(self.thresholds, m["fscore"])] + [("HD", m["hausdorff"])]


def check_alpha_option(opt, flag) -> None:
    """``--dcd`` here and ``--dcd_alpha`` of the training options (``cli.validate``)."""
    alpha = getattr(opt, flag, None)
    if alpha is not None:
        try:
            metrics.check_dcd_alpha(alpha)
        except ValueError as e:
            raise SystemExit(f"--{flag}: {e}") from None


class Dcd(Column):
    """``--dcd [ALPHA]``: the density-aware Chamfer distance (K18 over K1's minima and indices, in [0, 1]), averaged over
    an item's queries on the device and then over the class's items."""

    needs_rows = True

    def __init__(self, alpha):
        self.alpha = metrics.check_dcd_alpha(alpha)
        self.result = defaultdict(list)

    @staticmethod
    def add_arguments(group):
        group.add_argument("--dcd", type=float, nargs="?", const=1000.0, default=None, metavar="ALPHA",
                           help="Also report per class the density-aware Chamfer distance of the reconstructions (in "
                                "[0, 1]; HIP, fpsg_amd.metrics.dcd); ALPHA is the factor on the squared distance "
                                "[default: 1000];")

    @staticmethod
    def check(opt):
        check_alpha_option(opt, "dcd")

    @classmethod
    def from_options(cls, opt):
        alpha = getattr(opt, "dcd", None)
        return None if alpha is None else cls(alpha)

    def item_options(self):
        return {"dcd": self.alpha}

    def per_item(self, syn_pc, ref_pc_q, rows):
        return {"dcd": metrics.dcd_from_rows(rows, self.alpha).mean()}

    def add(self, name, out, n_query):
        self.result[name].append(out["dcd"].item())

    def fields(self, name):
        return [("DCD", statistics.mean(self.result[name]))]


class _SetColumn(Column):
    """MMD, COV and 1-NNA over all generated and reference query clouds of a class, which stay on the device until the
    class is finished.  ``--set_metrics_points N`` is an option of both groups: the clouds are first reduced to ``N``
    points each by farthest point sampling from index 0 (K16, two launches per item, only the reduced clouds are kept)
    and the labels end in ``@N``."""

    flag = generate = None                  # the option's name; the name of the ``set_metrics`` function
    keys = labels = ()                      # of that function's dict; of the line

    def __init__(self, points=None):
        self.points = points
        self.gen, self.ref = defaultdict(list), defaultdict(list)
        self.result = {}

    @staticmethod
    def add_points_argument(group):
        group.add_argument("--set_metrics_points", type=int, default=None, metavar="N",
                           help="With --set_metrics / --set_metrics_emd: reduce every generated and reference query cloud "
                                "to N points by farthest point sampling from index 0 (HIP, fpsg_amd.sampling) before the "
                                "set metrics; the labels become MMD-CD@N, ...; every other column stays on the full "
                                "clouds;")

    @staticmethod
    def check(opt):
        points = getattr(opt, "set_metrics_points", None)
        if points is not None:
            if not (getattr(opt, "set_metrics", False) or getattr(opt, "set_metrics_emd", False)):
                raise SystemExit("--set_metrics_points needs --set_metrics and / or --set_metrics_emd")
            if points < 1:
                raise SystemExit(f"--set_metrics_points must be at least 1 (got {points})")

    @classmethod
    def from_options(cls, opt):
        return cls(getattr(opt, "set_metrics_points", None)) if getattr(opt, cls.flag, False) else None

    def add(self, name, out, n_query):
        if "set_clouds" not in out:         # reduced once per item, however many groups read them
            gen, ref = out["syn_pc"], out["ref_pc_q"]
            if self.points is not None:
                for which, c in (("generated", gen), ("reference", ref)):
                    if self.points > c.size(1):
                        raise ValueError(f"--set_metrics_points {self.points} exceeds the {c.size(1)} points of the "
                                         f"{which} clouds")
                gen = sampling.farthest_point_subsample(gen.contiguous(), self.points, start=0)
                ref = sampling.farthest_point_subsample(ref.contiguous(), self.points, start=0)
            out["set_clouds"] = gen, ref
        gen, ref = out["set_clouds"]
        self.gen[name].append(gen)
        self.ref[name].append(ref)

    def finish(self):
        for name in sorted(self.gen):
            self.result[name] = getattr(set_metrics, self.generate)(torch.cat(self.gen[name]), torch.cat(self.ref[name]))

    def fields(self, name):
        at = "" if self.points is None else f"@{self.points}"
        return [(label + at, self.result[name][key]) for label, key in zip(self.labels, self.keys)]


class SetMetricsCd(_SetColumn):
    """``--set_metrics``: under the Chamfer distance, from K13's matrices."""

    flag, generate = "set_metrics", "generation_metrics"
    keys, labels = ("mmd_cd", "cov_cd", "nna_cd"), ("MMD-CD", "COV-CD", "1-NNA-CD")

    @staticmethod
    def add_arguments(group):
        group.add_argument("--set_metrics", action="store_true",
                           help="Also report MMD-CD, COV-CD and 1-NNA-CD per class over all its generated and reference "
                                "query clouds (HIP Chamfer matrix, fpsg_amd.set_metrics);")


class SetMetricsEmd(_SetColumn):
    """``--set_metrics_emd``: under the exact EMD, from K14's matrices; ``EMD-uncertified: <cov>/<nna>`` follows when
    some nearest-neighbour decisions are not certified by the EMD bounds."""

    flag, generate = "set_metrics_emd", "emd_generation_metrics"
    keys, labels = ("mmd_emd", "cov_emd", "nna_emd"), ("MMD-EMD", "COV-EMD", "1-NNA-EMD")

    @staticmethod
    def add_arguments(group):
        group.add_argument("--set_metrics_emd", action="store_true",
                           help="Also report MMD-EMD, COV-EMD and 1-NNA-EMD per class over all its generated and "
                                "reference query clouds (HIP exact EMD matrix, fpsg_amd.set_metrics);")
        _SetColumn.add_points_argument(group)       # behind the two flags it belongs to

    def fields(self, name):
        m = self.result[name]
        uncertified = [("EMD-uncertified", f"{m['cov_uncertified']}/{m['nna_uncertified']}")]
        return super().fields(name) + (uncertified if m["cov_uncertified"] or m["nna_uncertified"] else [])


class Jsd(Column):
    """``--jsd``: the Jensen-Shannon divergence between the voxel-occupancy distributions of the class's generated and
    reference query clouds, from K15's grids: two launches per item accumulate into them, no cloud is kept."""

    def __init__(self):
        self.grid_gen, self.grid_ref = {}, {}
        self.result = {}

    @staticmethod
    def add_arguments(group):
        group.add_argument("--jsd", action="store_true",
                           help="Also report the Jensen-Shannon divergence per class between the voxel-occupancy "
                                "distributions of its generated and reference query clouds (HIP occupancy grid, "
                                "fpsg_amd.set_metrics.jsd);")

    @classmethod
    def from_options(cls, opt):
        return cls() if getattr(opt, "jsd", False) else None

    def add(self, name, out, n_query):
        self.grid_gen[name] = metrics.occupancy_grid(out["syn_pc"].contiguous(), out=self.grid_gen.get(name))
        self.grid_ref[name] = metrics.occupancy_grid(out["ref_pc_q"].contiguous(), out=self.grid_ref.get(name))

    def finish(self):
        for name in sorted(self.grid_gen):
            self.result[name] = set_metrics.jsd_from_grids(self.grid_gen[name], self.grid_ref[name])

    def fields(self, name):
        return [("JSD", self.result[name]["jsd"])]


# The two fixed orders.  A class's line reads ``Rec CD; Rec EMD`` and then the active groups in the order of COLUMNS.
# ``main`` returns ``(per_class_cd, per_class_emd)`` and then one element per active group in RETURN_ORDER, the order in
# which the groups were added (callers index the tuple by it); the command line lists and checks them in that order too.
COLUMNS = (ExactEmd, FScore, Dcd, SetMetricsCd, SetMetricsEmd, Jsd)
RETURN_ORDER = (ExactEmd, SetMetricsCd, SetMetricsEmd, Jsd, FScore, Dcd)


def add_arguments(group) -> None:
    for cls in RETURN_ORDER:
        cls.add_arguments(group)


def check(opt) -> None:
    for cls in RETURN_ORDER:
        cls.check(opt)


def active_columns(opt) -> list:
    """The groups ``opt`` asks for, in line order."""
    return [c for c in (cls.from_options(opt) for cls in COLUMNS) if c is not None]


def item_columns(exact_emd: bool = False, fscore=None, dcd=None) -> list:
    """The groups with a per-item part that ``EvalItem``'s keywords switch on, in line order."""
    return ([ExactEmd()] if exact_emd else []) + ([] if fscore is None else [FScore(fscore)]) + \
        ([] if dcd is None else [Dcd(dcd)])


def item_options(columns) -> dict:
    """The keywords to open ``EvalItem`` with for these groups."""
    return {k: v for c in columns for k, v in c.item_options().items()}


def line(name, cd, emd, columns) -> str:
    fields = [("Rec CD", cd), ("Rec EMD", emd)] + [f for c in columns for f in c.fields(name)]
    return f"Class: {name} -- " + "; ".join(f"{label}: {value}" for label, value in fields)


def results(columns) -> tuple:
    """One per-class object per active group, in RETURN_ORDER."""
    return tuple(c.result for cls in RETURN_ORDER for c in columns if type(c) is cls)
