"""The conditions under which tests/test_trajectory_gpu.py can see stale cross-step state, established on the reference
alone (the fp32 CPU port, five Adam steps at the trajectory shape of tests/_trajectory_ref.py).

They are conditions on the INPUTS, not tolerances of any code under test: a weight that is one optimizer step out of
date must move the losses by far more than the bounds the GPU test allows.  If a change of the shape, the learning rate
or the episodes breaks one of them, change the inputs (``_trajectory_ref.LR`` is shared by both files), not the floors."""
import re
import statistics

import pytest
import torch

import _trajectory_ref as tr

STEPS = 5
# 4 clusters of 4 patches: patch 0 is cluster 0's node 0 behind cluster 0's deformer, patch 15 cluster 3's node 3 behind
# cluster 3's deformer
PATCHES_0_AND_15 = re.compile(r"cluster_pool\.(0\.(deformer|node_pool\.0)|3\.(deformer|node_pool\.3))\.")


@pytest.fixture(scope="module")
def run():
    """Five steps of the fp32 CPU port; ``snaps[t]`` is the model's state in front of step ``t``."""
    from fpsg_amd.engine import build_model
    torch.manual_seed(0)
    template = build_model(tr.options(device="cpu"))
    grids = tr.fixed_grids(template, (tr.S, tr.Q), "cpu")
    model = tr.cpu_reference(template, grids)
    eps = [tr.episode(k) for k in range(STEPS)]
    optimizer = torch.optim.Adam(model.parameters(), lr=tr.LR)
    snaps, losses = [], []
    for ep in eps:
        snaps.append(tr.copy_state(model.state_dict()))
        out = model.loss(ep)
        optimizer.zero_grad()
        out["ttl_loss"].sum().backward()
        optimizer.step()
        losses.append(tr.losses_of(out))
    probe = tr.cpu_reference(template, grids)

    def loss_with(state, ep):
        probe.load_state_dict(state)
        probe.train()
        with torch.no_grad():
            return tr.losses_of(probe.loss(ep))

    return {"template": template, "grids": grids, "eps": eps, "snaps": snaps, "losses": losses, "loss_with": loss_with}


def test_the_run_trains(run):
    """Adam at this learning rate moves every loss from step to step (a trajectory that stood still could hide anything)."""
    ttl = [l["ttl_loss"] for l in run["losses"]]
    print("ttl_loss per step:", ttl)
    assert all(v > 0 and v == v for v in ttl) and len(set(ttl)) == STEPS


def test_group_sensitivity(run):
    """Episode ``t`` evaluated with ONE module group's parameters taken from snapshot ``t - 1``: ``ttl_loss`` moves by at
    least ``GROUP_FLOOR`` relative, for every group and every ``t >= 1``."""
    worst = {}
    for t in range(1, STEPS):
        fresh = run["loss_with"](run["snaps"][t], run["eps"][t])["ttl_loss"]
        for g in tr.GROUPS:
            state = dict(run["snaps"][t])
            for k in state:
                if k.startswith(g) and tr.is_weight(k):
                    state[k] = run["snaps"][t - 1][k]
            moved = abs(run["loss_with"](state, run["eps"][t])["ttl_loss"] - fresh) / abs(fresh)
            print(f"step {t}: {g} one step out of date moves ttl_loss by {moved:.3e}")
            worst[g] = min(worst.get(g, moved), moved)
    print("group sensitivity, smallest per group:", worst)
    assert min(worst.values()) >= tr.GROUP_FLOOR, worst


def test_single_tensor_sensitivity(run):
    """The same for ONE weight tensor of two or more dimensions -- every convolution of the image encoder, the point
    encoder, patches 0 and 15 of the decoder with their clusters' deformers -- for every ``t >= 1``: the worse-moved of
    ``query_rec_loss`` and ``support_rec_loss`` moves by at least ``SINGLE_TENSOR_FLOOR`` relative.  The floor is what
    holds for the least sensitive kind of tensor, a deformer's first layer (2 input channels); every other kind is held to
    ``SINGLE_TENSOR_FLOOR_WITHOUT_DEFORMER_INPUT``, ten times higher."""
    names = [k for k, v in run["snaps"][0].items()
             if tr.is_weight(k) and k.endswith("weight") and v.dim() >= 2
             and (not k.startswith("pc_decoder") or PATCHES_0_AND_15.search(k))]
    assert sum(k.startswith("img_encoder") for k in names) >= 3 and sum(k.startswith("pc_encoder") for k in names) >= 3
    for part in ("cluster_pool.0.node_pool.0.", "cluster_pool.3.node_pool.3.", "cluster_pool.0.deformer.conv1.",
                 "cluster_pool.3.deformer.conv1."):
        assert any(part in k for k in names), part
    smallest = smallest_other = None
    for t in range(1, STEPS):
        fresh = run["loss_with"](run["snaps"][t], run["eps"][t])
        res = []
        for k in names:
            assert not torch.equal(run["snaps"][t][k], run["snaps"][t - 1][k]), k      # no frozen layer: all can be stale
            state = dict(run["snaps"][t])
            state[k] = run["snaps"][t - 1][k]
            got = run["loss_with"](state, run["eps"][t])
            res.append((max(abs(got[q] - fresh[q]) / abs(fresh[q]) for q in ("query_rec_loss", "support_rec_loss")), k))
        res.sort()
        other = [r for r in res if "deformer.conv1." not in r[1]]
        conv = [r for r in res if r[1].startswith("img_encoder")]
        print(f"step {t}: {len(res)} tensors; smallest {res[:3]}; smallest but a deformer's first layer {other[0]}; "
              f"median {statistics.median(r[0] for r in res):.3e}; smallest image-encoder convolution {conv[0]}")
        assert len(res) >= 30
        smallest = res[0] if smallest is None else min(smallest, res[0])
        smallest_other = other[0] if smallest_other is None else min(smallest_other, other[0])
    print("single-tensor sensitivity, smallest:", smallest, "; but a deformer's first layer:", smallest_other)
    assert smallest[0] >= tr.SINGLE_TENSOR_FLOOR, smallest
    assert smallest_other[0] >= tr.SINGLE_TENSOR_FLOOR_WITHOUT_DEFORMER_INPUT, smallest_other
    # what this floor allows the GPU test: a loss bound of a tenth of it
    assert tr.RESTART_LOSS_BOUND_CAP <= smallest[0] / 10


def test_reference_deviation(run):
    """The fp32 CPU port against the same model in float64 at every snapshot: every loss within
    ``REFERENCE_DEVIATION_CAP`` relative, so that three times it stays under a quarter of the group floor."""
    m64 = tr.cpu_reference(run["template"], run["grids"], torch.float64)
    worst = {}
    for t in range(STEPS):
        a = run["loss_with"](run["snaps"][t], run["eps"][t])
        m64.load_state_dict(run["snaps"][t])
        m64.train()
        with torch.no_grad():
            b = tr.losses_of(m64.loss(tr.episode_to(run["eps"][t], dtype=torch.float64)))
        dev = {k: abs(a[k] - b[k]) / abs(b[k]) for k in tr.LOSS_KEYS}
        print(f"snapshot {t}: fp32 CPU port vs float64 {dev}")
        for k, v in dev.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("reference deviation, largest per loss:", worst)
    assert max(worst.values()) <= tr.REFERENCE_DEVIATION_CAP, worst
    assert tr.MARGIN * tr.REFERENCE_DEVIATION_CAP <= tr.FLOAT64_LOSS_BOUND_CAP
