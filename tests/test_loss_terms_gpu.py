"""The regularisers in ``ImgPCProtoNet.loss`` bit for bit: with the repulsion, expansion and uniform terms all on, the keys
enter the dict in that order, each ``*_loss`` entry is the unweighted sum of the values its function returned, and
``ttl_loss`` is ``recon_loss`` with the weighted terms added one after the other in that order.  Float addition order is
observable, so everything is compared with ``torch.equal`` against the same torch operations on the device; the model-level
tests of the single terms compare to 1e-6 and would not see a reordering."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BASE_KEYS = ["ttl_loss", "recon_loss", "query_rec_loss", "support_rec_loss"]
TERMS = (("repulsion_loss", "repulsion_loss", 0.25), ("expansion_penalty", "expansion_loss", 0.125),
         ("uniform_loss", "uniform_loss", 0.5))                      # (few_shot's name, the dict key, the weight)
QUERY_FACTOR, SUPPORT_FACTOR = 1.0, 0.75


@pytest.mark.parametrize("intra_recon", [True, False])
@pytest.mark.parametrize("pc_dist", ["cd", "dcd"])
def test_terms_are_added_in_table_order_bit_for_bit(gpu, monkeypatch, pc_dist, intra_recon):
    """``cd`` takes the fused K1l path, ``dcd`` the batched one; without ``intra_recon`` there is no support part."""
    from fpsg_amd import few_shot
    from fpsg_amd.engine import build_model, default_options
    from fpsg_amd.episodes import synthetic_episode
    S, Q = 2, 1
    torch.manual_seed(5)
    model = build_model(default_options(
        device="cuda", pc_dist=pc_dist, intra_recon=intra_recon, n_shot=S, n_query=Q, query_factor=QUERY_FACTOR,
        support_factor=SUPPORT_FACTOR, repulsion_weight=0.25, expansion_weight=0.125, uniform_weight=0.5,
        uniform_percentages=(0.01, 0.03), uniform_radius=0.5)).to(gpu).train()
    seen = {}

    def spy_on(name):
        inner = getattr(few_shot, name)

        def spy(p, *args, **kwargs):
            value = inner(p, *args, **kwargs)
            seen.setdefault(name, []).append((p.detach().clone(), value))
            return value

        monkeypatch.setattr(few_shot, name, spy)

    for name, _, _ in TERMS:
        spy_on(name)
    ep = synthetic_episode(S, Q, n_pts=2048, img_size=96, seed=52, device=gpu)
    torch.manual_seed(13)                                            # the decoder's random grid
    out = model.loss(ep)

    assert list(out) == BASE_KEYS + [key for _, key, _ in TERMS]
    n_clouds = Q + S if intra_recon else Q
    first = seen[TERMS[0][0]][0][0]
    assert tuple(first.shape) == (n_clouds, 2048, 3)
    want = out["recon_loss"].detach()
    for name, key, weight in TERMS:
        assert len(seen[name]) == 1, f"ONE {name} call over the decoded clouds"
        clouds, value = seen[name][0]
        assert torch.equal(clouds, first), f"{name} saw other clouds than {TERMS[0][0]}"
        v = value.detach()
        assert tuple(v.shape) == (n_clouds,)
        q_sum = v[:Q].sum()
        weighted, total = QUERY_FACTOR * q_sum, q_sum
        if intra_recon:
            s_sum = v[Q:].sum()
            weighted, total = weighted + SUPPORT_FACTOR * s_sum, total + s_sum
        assert torch.equal(out[key].detach(), total), key
        want = want + weight * weighted
    assert bool(torch.isfinite(want).all())
    assert torch.equal(out["ttl_loss"].detach(), want), (out["ttl_loss"], want)
    assert not torch.equal(out["ttl_loss"].detach(), out["recon_loss"].detach())
