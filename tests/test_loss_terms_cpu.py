"""The loss terms' host code, which needs no GPU: (a) every loss option has ONE default -- ``few_shot.LOSS_OPTION_DEFAULTS``
-- and the model's signature, ``engine.default_options`` and the parser agree with it; (b) an options namespace from
before any of those options existed builds the default model; (c) every message of the option checks and of
``cli.validate`` is, character for character, what it was when the checks were written out one by one (the texts below
were recorded from that code; the CLI forwards them, so they are part of the command line's behaviour)."""
import argparse
import inspect
import math

import pytest
import torch

LOSS_OPTIONS = ("dcd_alpha", "sinkhorn_blur", "sinkhorn_diameter", "swd_n_proj", "swd_directions", "repulsion_weight",
                "repulsion_k", "repulsion_h", "expansion_weight", "expansion_lambda", "uniform_weight",
                "uniform_percentages", "uniform_radius")


# ---- (a) one default per option ------------------------------------------------------------------------------------------

def _same(a, b):
    return type(a) is type(b) and a == b


def test_the_table_names_the_thirteen_options():
    from fpsg_amd.few_shot import LOSS_OPTION_DEFAULTS
    assert tuple(LOSS_OPTION_DEFAULTS) == LOSS_OPTIONS


@pytest.mark.parametrize("name", LOSS_OPTIONS)
def test_defaults_agree(name):
    from fpsg_amd import cli
    from fpsg_amd.engine import default_options
    from fpsg_amd.few_shot import LOSS_OPTION_DEFAULTS, ImgPCProtoNet
    want = LOSS_OPTION_DEFAULTS[name]
    signature = inspect.signature(ImgPCProtoNet.__init__).parameters[name].default
    assert signature is not inspect.Parameter.empty and _same(signature, want), (signature, want)
    assert _same(getattr(default_options(), name), want)
    for evaluation in (False, True):
        parsed = cli.few_shot_parser(evaluation=evaluation).parse_args([])
        if name == "uniform_percentages":
            assert not hasattr(parsed, name)                         # the flag is in percent; validate() converts
            assert _same(cli.uniform_fractions(parsed.uniform_percent), want)
        else:
            assert _same(getattr(parsed, name), want), (getattr(parsed, name), want)


# ---- (b) a namespace from before the options -----------------------------------------------------------------------------

def test_a_stripped_namespace_builds_the_default_model():
    from fpsg_amd.engine import build_model, default_options
    full = default_options(device="cpu")
    old = argparse.Namespace(**{k: v for k, v in vars(full).items() if k not in LOSS_OPTIONS})
    assert not any(hasattr(old, n) for n in LOSS_OPTIONS)
    seen = set()
    for pc_dist in ("dcd", "sinkhorn", "swd"):                       # a distance's own options exist only under it
        old.pc_dist = full.pc_dist = pc_dist
        built, default = build_model(old), build_model(full)
        have = [n for n in LOSS_OPTIONS if hasattr(default, n)]
        assert [n for n in LOSS_OPTIONS if hasattr(built, n)] == have
        for n in have:
            assert _same(getattr(built, n), getattr(default, n)), n
        seen |= set(have)
    assert seen == set(LOSS_OPTIONS)


# ---- (c) the messages ------------------------------------------------------------------------------------------------------

# (flag, bad value, what cli.validate exits with) on the namespace of `--synthetic`
CLI_MESSAGES = [
    ('repulsion_weight', -1.0, '--repulsion_weight must be finite and non-negative, got -1.0'),
    ('expansion_weight', math.nan, '--expansion_weight must be finite and non-negative, got nan'),
    ('uniform_weight', 'x', "--uniform_weight must be a number, got 'x'"),
    ('repulsion_weight', True, '--repulsion_weight must be finite and non-negative, got True'),
    ('ema_decay', 1.5, '--ema_decay: a number in [0, 1) or None, got 1.5'),
    ('ema_decay', 'x', "--ema_decay: a number in [0, 1) or None, got 'x'"),
    ('repulsion_k', 9, '--repulsion_k must be in 1..8, got 9'),
    ('repulsion_k', True, '--repulsion_k must be an integer in 1..8, got True'),
    ('repulsion_k', 2.0, '--repulsion_k must be an integer in 1..8, got 2.0'),
    ('repulsion_h', 0.0, '--repulsion_h must be positive and finite, got 0.0'),
    ('repulsion_h', 'x', "--repulsion_h must be a number, got 'x'"),
    ('expansion_lambda', 0.5, '--expansion_lambda: lam must be finite and at least 1, got 0.5'),
    ('expansion_lambda', 'x', "--expansion_lambda: lam must be a number, got 'x'"),
    ('expansion_lambda', True, '--expansion_lambda: lam must be finite and at least 1, got True'),
    ('uniform_percent', [100.5], '--uniform_percent: each value must be in (0, 100], got 100.5'),
    ('uniform_percent', [], '--uniform_percent: 1..8 values, got 0'),
    ('uniform_percent', ['x'], "--uniform_percent: 1..8 numbers in (0, 100], got ['x']"),
    ('uniform_radius', 0.0, '--uniform_radius must be positive and finite, got 0.0'),
    ('uniform_radius', 'x', "--uniform_radius must be a number, got 'x'"),
    ('uniform_radius', True, '--uniform_radius must be positive and finite, got True'),
    ('swd_n_proj', 0, '--swd_n_proj must be in 1..1024, got 0'),
    ('swd_n_proj', True, '--swd_n_proj must be an integer in 1..1024, got True'),
    ('swd_n_proj', 1.5, '--swd_n_proj must be an integer in 1..1024, got 1.5'),
    ('swd_directions', 'both', "--swd_directions must be one of ('random', 'fixed'), got 'both'"),
    ('sinkhorn_blur', 0.0, '--sinkhorn_blur must be finite and positive, got 0.0'),
    ('sinkhorn_diameter', 'x', "--sinkhorn_diameter must be a number, got 'x'"),
    ('sinkhorn_diameter', math.inf, '--sinkhorn_diameter must be finite and positive, got inf'),
    ('dcd_alpha', -1.0, '--dcd_alpha: alpha must be finite and non-negative, got -1.0'),
    ('dcd_alpha', 'x', "--dcd_alpha: alpha must be a number, got 'x'"),
]

# several bad values at once: the check that comes first in validate() reports
FIRST_ERRORS = [
    ({'repulsion_weight': -1.0, 'swd_n_proj': 0, 'ema_decay': 2.0}, '--swd_n_proj must be in 1..1024, got 0'),
    ({'repulsion_weight': -1.0, 'repulsion_k': 0, 'uniform_radius': 0.0}, '--repulsion_weight must be finite and non-negative, got -1.0'),
    ({'repulsion_h': 0.0, 'expansion_weight': -2.0}, '--repulsion_h must be positive and finite, got 0.0'),
    ({'expansion_lambda': 0.0, 'uniform_weight': -1.0}, '--expansion_lambda: lam must be finite and at least 1, got 0.0'),
    ({'uniform_percent': [0.0], 'uniform_radius': 0.0, 'ema_decay': 2.0}, '--uniform_percent: each value must be in (0, 100], got 0.0'),
    ({'sinkhorn_diameter': 0.0, 'sinkhorn_blur': 0.0, 'dcd_alpha': -1.0}, '--dcd_alpha: alpha must be finite and non-negative, got -1.0'),
    ({'sinkhorn_diameter': 0.0, 'swd_n_proj': 0}, '--sinkhorn_diameter must be finite and positive, got 0.0'),
]

# (function, bad arguments, the ValueError's text); the tensors are CPU tensors: these refusals come before any GPU work
CHECKER_MESSAGES = [
    ('metrics.check_dcd_alpha', ('x',), "alpha must be a number, got 'x'"),
    ('metrics.check_dcd_alpha', (None,), 'alpha must be a number, got None'),
    ('metrics.check_dcd_alpha', (-1.0,), 'alpha must be finite and non-negative, got -1.0'),
    ('metrics.check_dcd_alpha', (math.inf,), 'alpha must be finite and non-negative, got inf'),
    ('metrics.check_dcd_alpha', (math.nan,), 'alpha must be finite and non-negative, got nan'),
    ('metrics.check_repulsion_options', ('4', 0.03), "k must be an integer in 1..8, got '4'"),
    ('metrics.check_repulsion_options', (4.0, 0.03), 'k must be an integer in 1..8, got 4.0'),
    ('metrics.check_repulsion_options', (True, 0.03), 'k must be an integer in 1..8, got True'),
    ('metrics.check_repulsion_options', (0, 0.03), 'k must be in 1..8, got 0'),
    ('metrics.check_repulsion_options', (9, 0.03), 'k must be in 1..8, got 9'),
    ('metrics.check_repulsion_options', (4, 'x'), "h must be a number, got 'x'"),
    ('metrics.check_repulsion_options', (4, None), 'h must be a number, got None'),
    ('metrics.check_repulsion_options', (4, 0.0), 'h must be positive and finite, got 0.0'),
    ('metrics.check_repulsion_options', (4, -1.0), 'h must be positive and finite, got -1.0'),
    ('metrics.check_repulsion_options', (4, True), 'h must be positive and finite, got True'),
    ('metrics.check_repulsion_options', (4, math.nan), 'h must be positive and finite, got nan'),
    ('metrics.check_repulsion_options', (4, math.inf), 'h must be positive and finite, got inf'),
    ('metrics.check_repulsion_options', (0, 'x'), 'k must be in 1..8, got 0'),
    ('metrics.check_expansion_options', (2.0, 1.5), 'patch_size must be an integer in 2..1024, got 2.0'),
    ('metrics.check_expansion_options', ('2', 1.5), "patch_size must be an integer in 2..1024, got '2'"),
    ('metrics.check_expansion_options', (True, 1.5), 'patch_size must be an integer in 2..1024, got True'),
    ('metrics.check_expansion_options', (1, 1.5), 'patch_size must be in 2..1024, got 1'),
    ('metrics.check_expansion_options', (1025, 1.5), 'patch_size must be in 2..1024, got 1025'),
    ('metrics.check_expansion_options', (2, 'x'), "lam must be a number, got 'x'"),
    ('metrics.check_expansion_options', (2, None), 'lam must be a number, got None'),
    ('metrics.check_expansion_options', (2, 0.5), 'lam must be finite and at least 1, got 0.5'),
    ('metrics.check_expansion_options', (2, True), 'lam must be finite and at least 1, got True'),
    ('metrics.check_expansion_options', (2, math.inf), 'lam must be finite and at least 1, got inf'),
    ('metrics.check_expansion_options', (2, math.nan), 'lam must be finite and at least 1, got nan'),
    ('metrics.check_expansion_options', (1, 'x'), 'patch_size must be in 2..1024, got 1'),
    ('metrics.check_uniform_options', (None, 1.0), 'percentages must be a sequence of 1..8 fractions in (0, 1], got None'),
    ('metrics.check_uniform_options', (0.01, 1.0), 'percentages must be a sequence of 1..8 fractions in (0, 1], got 0.01'),
    ('metrics.check_uniform_options', ('0.01', 1.0), "percentages must be a sequence of 1..8 fractions in (0, 1], got '0.01'"),
    ('metrics.check_uniform_options', (True, 1.0), 'percentages must be a sequence of 1..8 fractions in (0, 1], got True'),
    ('metrics.check_uniform_options', ((), 1.0), 'percentages must hold 1..8 values, got 0'),
    ('metrics.check_uniform_options', ((0.01,) * 9, 1.0), 'percentages must hold 1..8 values, got 9'),
    ('metrics.check_uniform_options', (('x',), 1.0), "percentages must be numbers, got 'x'"),
    ('metrics.check_uniform_options', ((None,), 1.0), 'percentages must be numbers, got None'),
    ('metrics.check_uniform_options', ((True,), 1.0), 'percentages must be in (0, 1], got True'),
    ('metrics.check_uniform_options', ((1.5,), 1.0), 'percentages must be in (0, 1], got 1.5'),
    ('metrics.check_uniform_options', ((0.0,), 1.0), 'percentages must be in (0, 1], got 0.0'),
    ('metrics.check_uniform_options', ((math.nan,), 1.0), 'percentages must be in (0, 1], got nan'),
    ('metrics.check_uniform_options', ((0.01,), 'x'), "radius must be a number, got 'x'"),
    ('metrics.check_uniform_options', ((0.01,), None), 'radius must be a number, got None'),
    ('metrics.check_uniform_options', ((0.01,), 0.0), 'radius must be positive and finite, got 0.0'),
    ('metrics.check_uniform_options', ((0.01,), True), 'radius must be positive and finite, got True'),
    ('metrics.check_uniform_options', ((0.01,), math.inf), 'radius must be positive and finite, got inf'),
    ('metrics.check_uniform_options', ((2.0,), 0.0), 'percentages must be in (0, 1], got 2.0'),
    ('metrics.check_swd_options', (1.5, 'random'), 'n_proj must be an integer in 1..1024, got 1.5'),
    ('metrics.check_swd_options', ('64', 'random'), "n_proj must be an integer in 1..1024, got '64'"),
    ('metrics.check_swd_options', (True, 'random'), 'n_proj must be an integer in 1..1024, got True'),
    ('metrics.check_swd_options', (0, 'random'), 'n_proj must be in 1..1024, got 0'),
    ('metrics.check_swd_options', (1025, 'random'), 'n_proj must be in 1..1024, got 1025'),
    ('metrics.check_swd_options', (64, 'both'), "directions must be one of ('random', 'fixed'), got 'both'"),
    ('metrics.check_swd_options', (64, None), "directions must be one of ('random', 'fixed'), got None"),
    ('metrics.check_swd_options', (0, 'both'), 'n_proj must be in 1..1024, got 0'),
    ('metrics.check_sinkhorn_option', ('x', 'sinkhorn_blur'), "sinkhorn_blur must be a number, got 'x'"),
    ('metrics.check_sinkhorn_option', (None, 'sinkhorn_diameter'), 'sinkhorn_diameter must be a number, got None'),
    ('metrics.check_sinkhorn_option', (0.0, 'sinkhorn_blur'), 'sinkhorn_blur must be finite and positive, got 0.0'),
    ('metrics.check_sinkhorn_option', (-1.0, 'sinkhorn_diameter'), 'sinkhorn_diameter must be finite and positive, got -1.0'),
    ('metrics.check_sinkhorn_option', (math.inf, 'sinkhorn_blur'), 'sinkhorn_blur must be finite and positive, got inf'),
    ('metrics.check_sinkhorn_option', (math.nan, 'sinkhorn_blur'), 'sinkhorn_blur must be finite and positive, got nan'),
    ('few_shot.check_repulsion_weight', ('x',), "repulsion_weight must be a number, got 'x'"),
    ('few_shot.check_repulsion_weight', (None,), 'repulsion_weight must be a number, got None'),
    ('few_shot.check_repulsion_weight', (-1.0,), 'repulsion_weight must be finite and non-negative, got -1.0'),
    ('few_shot.check_repulsion_weight', (True,), 'repulsion_weight must be finite and non-negative, got True'),
    ('few_shot.check_repulsion_weight', (math.nan,), 'repulsion_weight must be finite and non-negative, got nan'),
    ('few_shot.check_repulsion_weight', (math.inf,), 'repulsion_weight must be finite and non-negative, got inf'),
    ('few_shot.check_expansion_weight', ('x',), "expansion_weight must be a number, got 'x'"),
    ('few_shot.check_expansion_weight', (-0.5,), 'expansion_weight must be finite and non-negative, got -0.5'),
    ('few_shot.check_expansion_weight', (False,), 'expansion_weight must be finite and non-negative, got False'),
    ('few_shot.check_expansion_weight', (math.inf,), 'expansion_weight must be finite and non-negative, got inf'),
    ('few_shot.check_uniform_weight', ('x',), "uniform_weight must be a number, got 'x'"),
    ('few_shot.check_uniform_weight', (-2,), 'uniform_weight must be finite and non-negative, got -2'),
    ('few_shot.check_uniform_weight', (True,), 'uniform_weight must be finite and non-negative, got True'),
    ('few_shot.check_uniform_weight', (math.nan,), 'uniform_weight must be finite and non-negative, got nan'),
    ('metrics.repulsion_loss', (torch.zeros(2, 16, 2),), 'expected a [B,N,3] cloud tensor, got (2, 16, 2)'),
    ('metrics.repulsion_loss', (torch.zeros(16, 3),), 'expected a [B,N,3] cloud tensor, got (16, 3)'),
    ('metrics.repulsion_loss', (None,), 'expected a [B,N,3] cloud tensor, got ()'),
    ('metrics.repulsion_loss', (torch.zeros(0, 16, 3),), 'empty batches are not supported (got (0, 16, 3))'),
    ('metrics.repulsion_loss', (torch.zeros(2, 4, 3),), 'repulsion_loss needs at least k + 1 = 5 points per cloud, got 4'),
    ('metrics.repulsion_loss', (torch.zeros(2, 2, 3), 2), 'repulsion_loss needs at least k + 1 = 3 points per cloud, got 2'),
    ('metrics.repulsion_loss', (torch.zeros(1, 16385, 3),), 'repulsion_loss supports at most 16384 points per cloud, got 16385'),
    ('metrics.repulsion_loss', (torch.zeros(2, 16, 2), 9), 'k must be in 1..8, got 9'),
    ('metrics.repulsion_loss', (torch.zeros(0, 2, 3), 4, 0.0), 'h must be positive and finite, got 0.0'),
    ('metrics.expansion_penalty', (torch.zeros(2, 16, 2), 4), 'expected a [B,N,3] cloud tensor, got (2, 16, 2)'),
    ('metrics.expansion_penalty', (torch.zeros(16, 3), 4), 'expected a [B,N,3] cloud tensor, got (16, 3)'),
    ('metrics.expansion_penalty', (None, 4), 'expected a [B,N,3] cloud tensor, got ()'),
    ('metrics.expansion_penalty', (torch.zeros(0, 16, 3), 4), 'empty batches are not supported (got (0, 16, 3))'),
    ('metrics.expansion_penalty', (torch.zeros(2, 18, 3), 4), 'expansion_penalty needs a positive multiple of patch_size = 4 points per cloud, got 18'),
    ('metrics.expansion_penalty', (torch.zeros(2, 3, 3), 4), 'expansion_penalty needs a positive multiple of patch_size = 4 points per cloud, got 3'),
    ('metrics.expansion_penalty', (torch.zeros(1, 16388, 3), 4), 'expansion_penalty supports at most 16384 points per cloud, got 16388'),
    ('metrics.expansion_penalty', (torch.zeros(2, 16, 2), 1), 'patch_size must be in 2..1024, got 1'),
    ('metrics.uniform_loss', (torch.zeros(2, 16, 2),), 'expected a [B,N,3] cloud tensor, got (2, 16, 2)'),
    ('metrics.uniform_loss', (torch.zeros(16, 3),), 'expected a [B,N,3] cloud tensor, got (16, 3)'),
    ('metrics.uniform_loss', (None,), 'expected a [B,N,3] cloud tensor, got ()'),
    ('metrics.uniform_loss', (torch.zeros(0, 16, 3),), 'empty batches are not supported (got (0, 16, 3))'),
    ('metrics.uniform_loss', (torch.zeros(2, 1, 3),), 'uniform_loss needs at least 2 points per cloud, got 1'),
    ('metrics.uniform_loss', (torch.zeros(1, 16385, 3),), 'uniform_loss supports at most 16384 points per cloud, got 16385'),
    ('metrics.uniform_loss', (torch.zeros(2, 16, 2), (0.0,)), 'percentages must be in (0, 1], got 0.0'),
    ('metrics.uniform_loss', (torch.zeros(0, 1, 3), (0.5,), 0.0), 'radius must be positive and finite, got 0.0'),
]

# what the checks let through, with the returned types (bool passes as a number where it always did)
ACCEPTED = [
    ('metrics.check_dcd_alpha', (True,), 1.0),
    ('metrics.check_dcd_alpha', (3,), 3.0),
    ('metrics.check_sinkhorn_option', (True, 'sinkhorn_blur'), 1.0),
    ('metrics.check_sinkhorn_option', (2, 'sinkhorn_diameter'), 2.0),
    ('metrics.check_repulsion_options', (8, 1), (8, 1.0)),
    ('metrics.check_expansion_options', (1024, 1), (1024, 1.0)),
    ('metrics.check_uniform_options', ([1, 0.5], 2), ((1.0, 0.5), 2.0)),
    ('metrics.check_swd_options', (1024, 'fixed'), (1024, 'fixed')),
    ('few_shot.check_repulsion_weight', (3,), 3.0),
    ('few_shot.check_expansion_weight', (0,), 0.0),
    ('few_shot.check_uniform_weight', (0.5,), 0.5),
]


def _validate_text(changes):
    from fpsg_amd import cli
    opt = cli.few_shot_parser().parse_args(["--synthetic"])
    for flag, value in changes.items():
        setattr(opt, flag, value)
    with pytest.raises(SystemExit) as e:
        cli.validate(opt)
    return str(e.value)


@pytest.mark.parametrize("flag,bad,text", CLI_MESSAGES, ids=[f"{c[0]}-{c[1]!r}" for c in CLI_MESSAGES])
def test_validate_messages_are_unchanged(flag, bad, text):
    assert _validate_text({flag: bad}) == text


@pytest.mark.parametrize("changes,text", FIRST_ERRORS, ids=["+".join(c[0]) for c in FIRST_ERRORS])
def test_validate_reports_the_same_first_error(changes, text):
    assert _validate_text(changes) == text


def _resolve(name):
    from fpsg_amd import few_shot, metrics
    module, attr = name.split(".")
    return getattr({"metrics": metrics, "few_shot": few_shot}[module], attr)


@pytest.mark.parametrize("checker,args,text", CHECKER_MESSAGES,
                         ids=[f"{n}-{c[0].split('.')[1]}" for n, c in enumerate(CHECKER_MESSAGES)])
def test_checker_messages_are_unchanged(checker, args, text):
    with pytest.raises(ValueError) as e:
        _resolve(checker)(*args)
    assert str(e.value) == text


def _typed(value):
    return tuple(_typed(v) for v in value) if isinstance(value, tuple) else (type(value), value)


@pytest.mark.parametrize("checker,args,result", ACCEPTED, ids=[f"{n}-{c[0].split('.')[1]}" for n, c in enumerate(ACCEPTED)])
def test_checkers_return_the_same_values_and_types(checker, args, result):
    assert _typed(_resolve(checker)(*args)) == _typed(result)
