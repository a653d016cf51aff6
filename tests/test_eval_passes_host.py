"""The evaluation loop without a GPU: the one table of its options (host/cli.py: EVAL_OPTIONS, check_eval_options) and the ORDER of
the engine calls of `Seq2SeqAttNN.test()` (host/model.py, host/eval_passes.py) on a recording engine (tests/eval_recorder.py)."""
import re

import pytest

import tcar_amd  # noqa: F401
from tcar_amd.host import cli
from tcar_amd.host.model import Seq2SeqAttNN

import eval_recorder

# a value that every option accepts
VALID = dict(eval_panel=128, fresh_hours=48.0, cat_cap=2, shard_eval_panel=128, eval_sections=4, eval_related=5, eval_candidates=16,
             eval_shortlist=80, eval_diversity=1.5, shard_eval_shortlist=80, eval_mixed=1)


def _rules(opt, kind):
    return [r for r in opt.rules if r.kind == kind]


def _satisfied(opt):
    """the smallest request that turns `opt` on: its own value, the engine it takes, and what it needs (and what that needs)"""
    by_name = {o.name: o for o in cli.EVAL_OPTIONS}
    values = {opt.name: VALID[opt.name], "dp_mode": "sharded" if any(r.arg == "sharded" for r in _rules(opt, "engine")) else "replica"}
    for r in _rules(opt, "needs"):
        values.update({k: v for k, v in _satisfied(by_name[r.arg]).items() if k != "dp_mode"})
    return values


def _breaking(opt, rule):
    """the smallest requests that break `rule` of `opt` and no rule before it -> [(values, gpus)]"""
    ok = _satisfied(opt)
    if rule.kind == "type":
        return [({opt.name: "1"}, 1), ({opt.name: True}, 1), ({opt.name: None}, 1)]
    if rule.kind == "finite":
        return [(dict(ok, **{opt.name: v}), 1) for v in (-1.0, float("nan"), float("inf"), float("-inf"))]
    if rule.kind == "range":
        lo, hi, step = rule.arg
        bad = ([lo - 1 if lo - 1 else -1] if lo is not None else []) + ([hi + 1] if hi is not None else []) + ([lo + 1] if step else [])
        return [(dict(ok, **{opt.name: v}), 1) for v in bad]
    if rule.kind == "engine":                     # (without what it needs: under the other engine those would be refused first)
        return [({opt.name: VALID[opt.name], "dp_mode": "sharded" if rule.arg == "one" else "replica"}, 1)]
    if rule.kind == "one_process":
        return [(ok, 2), (ok, 8)]
    if rule.kind == "needs":
        return [({k: v for k, v in ok.items() if k != rule.arg}, 1), (dict(ok, **{rule.arg: 0}), 1)]
    assert rule.kind == "excludes"
    return [(dict(ok, **{rule.arg: VALID[rule.arg]}), 1)]


def test_every_evaluation_flag_comes_from_the_table_and_every_rule_refuses_with_its_own_text():
    names = [o.name for o in cli.EVAL_OPTIONS]
    assert names == ["eval_panel", "fresh_hours", "cat_cap", "shard_eval_panel", "eval_sections", "eval_related", "eval_candidates",
                     "eval_shortlist", "eval_diversity", "shard_eval_shortlist", "eval_mixed"]
    assert sorted(names) == sorted(VALID) and cli.EvalRequest._fields == tuple(names)
    ap = cli.build_parser()
    flags = {a.dest: a for a in ap._actions if re.match(r"(eval_|shard_eval_|fresh_hours$|cat_cap$)", a.dest)}
    assert sorted(flags) == sorted(names)
    off = ap.parse_args([])
    for o in cli.EVAL_OPTIONS:
        assert flags[o.name].help is o.help and flags[o.name].type is o.type and getattr(off, o.name) == 0, o.name
    assert {o.name: o.type for o in cli.EVAL_OPTIONS if o.type is not int} == {"fresh_hours": float, "eval_diversity": float}
    cli.check_eval_options({})                     # nothing named: everything off
    cli.check_eval_options(vars(off), gpus=off.gpus)
    cli.check_eval_options({"dp_mode": "sharded"}, gpus=8)
    n_rules = 0
    for o in cli.EVAL_OPTIONS:
        ok = _satisfied(o)
        cli.check_eval_options(ok)
        cli.check_eval_options(dict(ok, **{o.name: 0}))
        for rule in o.rules:
            n_rules += 1
            for values, gpus in _breaking(o, rule):
                with pytest.raises(ValueError) as e:
                    cli.check_eval_options(values, gpus=gpus)
                assert str(e.value) == rule.text, (o.name, rule.kind, values)
    assert n_rules == 36 and len({r.text for o in cli.EVAL_OPTIONS for r in o.rules}) == 36
    # a refusal names its own flag first, and the tables' bounds are the constants beside it
    assert all(r.text.startswith("--" + o.name + " ") for o in cli.EVAL_OPTIONS for r in o.rules)
    bounds = {o.name: [r.arg for r in _rules(o, "range")] for o in cli.EVAL_OPTIONS}
    assert bounds["eval_panel"] == bounds["shard_eval_panel"] == [(128, cli.MAX_PANEL, 128)]
    assert bounds["eval_sections"] == [(None, cli.MAX_SECTIONS, None), (0, None, None)] and bounds["eval_related"] == [(1, cli.MAX_RELATED, None)]
    assert bounds["eval_candidates"] == [(2, cli.MAX_CANDIDATES, None)]
    assert bounds["eval_shortlist"] == bounds["shard_eval_shortlist"] == [(65, cli.MAX_SHORTLIST, None)]


@pytest.mark.parametrize("values, gpus, first", [
    (dict(eval_panel=100, dp_mode="sharded"), 1, "--eval_panel streams the WHOLE catalog"),
    (dict(eval_panel=128, fresh_hours=-1.0, cat_cap=-1), 1, "--fresh_hours must be positive"),
    (dict(cat_cap=2, eval_sections=4), 1, "--cat_cap needs --eval_panel"),
    (dict(eval_sections=17, eval_candidates=1), 1, "--eval_sections must be in"),
    (dict(eval_related=65, eval_candidates=1, eval_diversity="1"), 1, "--eval_related must be in"),
    (dict(eval_candidates=16, eval_shortlist=80, dp_mode="sharded"), 1, "--eval_candidates scores candidate lists"),
    (dict(eval_shortlist=64, shard_eval_shortlist=64), 1, "--eval_shortlist must be in"),
    (dict(eval_diversity=1.5, shard_eval_shortlist=80), 1, "--eval_diversity needs --eval_shortlist"),
    (dict(shard_eval_shortlist=80, eval_mixed=1), 1, "--shard_eval_shortlist merges the shortlists"),
    (dict(eval_mixed=1, eval_candidates=16, eval_shortlist=80, eval_panel=128), 2, "--eval_mixed cannot be combined with --gpus > 1"),
    (dict(eval_mixed=1, eval_candidates=16, eval_shortlist=80, eval_panel=128), 1, "--eval_mixed cannot be combined with --eval_candidates"),
])
def test_a_request_that_breaks_two_rules_is_refused_with_the_earlier_one(values, gpus, first):
    """... by the command line's check, by a model's own resolver, and with the values the model was built with"""
    with pytest.raises(ValueError) as e:
        cli.check_eval_options(values, gpus=gpus)
    assert str(e.value).startswith(first)
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)
    with pytest.raises(ValueError) as e2:
        m._eval_request(dict(values, gpus=gpus))
    assert str(e2.value) == str(e.value)
    for k, v in values.items():
        setattr(m, k, v)
    m.dp_world = gpus
    with pytest.raises(ValueError) as e3:
        m._eval_request({"dp_mode": values.get("dp_mode", "replica")})
    assert str(e3.value) == str(e.value)


def test_the_resolver_takes_args_over_the_model_and_returns_every_option_in_its_type():
    m = Seq2SeqAttNN.__new__(Seq2SeqAttNN)         # (no attribute at all: everything off)
    assert m._eval_request({}) == cli.EvalRequest(*[o.type(0) for o in cli.EVAL_OPTIONS])
    m.eval_panel, m.fresh_hours, m.eval_related = 256, 24, 9
    req = m._eval_request({"eval_related": 0, "cat_cap": "3", "eval_shortlist": None, "eval_diversity": 0})
    assert req == cli.EvalRequest(eval_panel=256, fresh_hours=24.0, cat_cap=3, shard_eval_panel=0, eval_sections=0, eval_related=0,
                                  eval_candidates=0, eval_shortlist=0, eval_diversity=0.0, shard_eval_shortlist=0, eval_mixed=0)
    assert [type(v) for v in req] == [o.type for o in cli.EVAL_OPTIONS]
    m.dp_world = 2                                 # the ranks of the model count beside the gpus of the args
    with pytest.raises(ValueError, match="eval_mixed cannot be combined with --gpus > 1"):
        m._eval_request({"eval_mixed": 1})
    m.dp_world = 1
    assert m._eval_request({"eval_mixed": 1, "gpus": None}).eval_mixed == 1
    with pytest.raises(ValueError, match="eval_mixed cannot be combined with --gpus > 1"):
        m._eval_request({"eval_mixed": 1, "gpus": 2})


# The engine calls of test(), recorded from the loop as it was BEFORE it was built from passes (one method, its branches in line):
# the same recording engine, the same fold, the same seeds.  They are the order that must not move.
FIRST = dict(eval_panel=128, fresh_hours=48.0, eval_candidates=16, eval_shortlist=80, eval_diversity=1.5, eval_sections=3, eval_related=5)
FIRST_CALLS = [
    'set_item_keys',
    'set_categories',
    'reset_coverage',
    'upload B=5 T=2',
    'eval_step_streamed B=5 panel=128 window=[5] max_per_category=None',
    'eval_diversity lists=5 block=None',
    'score_candidates B=5 C=16',
    'recommend_two_stage B=5 T=2 shortlist=80 exclude_seen=False panel=128 window=[5] diversity=None',
    'recommend_two_stage B=5 T=2 shortlist=80 exclude_seen=False panel=128 window=[5] diversity=1.5',
    'recommend_sections B=5 T=2 G=3 k=20 exclude_seen=False panel=128 window=[5]',
    'upload B=2 T=1',
    'eval_step_streamed B=2 panel=128 window=[2] max_per_category=None',
    'eval_diversity lists=2 block=None',
    'score_candidates B=2 C=16',
    'recommend_two_stage B=2 T=1 shortlist=80 exclude_seen=False panel=128 window=[2] diversity=None',
    'recommend_two_stage B=2 T=1 shortlist=80 exclude_seen=False panel=128 window=[2] diversity=1.5',
    'recommend_sections B=2 T=1 G=3 k=20 exclude_seen=False panel=128 window=[2]',
    'upload B=8 T=1',
    'eval_step_streamed B=8 panel=128 window=[8] max_per_category=None',
    'eval_diversity lists=8 block=None',
    'score_candidates B=8 C=16',
    'recommend_two_stage B=8 T=1 shortlist=80 exclude_seen=False panel=128 window=[8] diversity=None',
    'recommend_two_stage B=8 T=1 shortlist=80 exclude_seen=False panel=128 window=[8] diversity=1.5',
    'recommend_sections B=8 T=1 G=3 k=20 exclude_seen=False panel=128 window=[8]',
    'check_forks',
    'coverage',
    'similar_items Q=8 k=5',
    'similar_items Q=3 k=5',
]
PACKED = dict(eval_panel=128, eval_mixed=1, cat_cap=2, eval_sections=3)
PACKED_CALLS = [
    'set_categories',
    'reset_coverage',
    'upload ragged B=7 R=12',
    'eval_step_streamed B=7 panel=128 window=none max_per_category=2',
    'eval_diversity lists=5 block=(0, 5, 2)',
    'eval_diversity lists=2 block=(10, 2, 1)',
    'recommend_sections ragged B=7 R=12 G=3 k=20 exclude_seen=False panel=128 window=none',
    'upload B=8 T=1',
    'eval_step_streamed B=8 panel=128 window=none max_per_category=2',
    'eval_diversity lists=8 block=(0, 8, 1)',
    'recommend_sections B=8 T=1 G=3 k=20 exclude_seen=False panel=128 window=none',
    'check_forks',
    'coverage',
]
CORE_KEYS = ["mrr", "recall", "ndcg", "loss", "ild", "unexp", "coverage", "eval_calls", "sessions"]


@pytest.fixture(scope="module")
def fold_and_data():
    return eval_recorder.fold_and_data()


def test_the_engine_calls_of_one_feed_keep_their_order_and_the_related_calls_come_behind_the_loop(fold_and_data, capsys):
    calls, metrics, recall = eval_recorder.recorded_test(Seq2SeqAttNN, *fold_and_data, **FIRST)
    assert calls == FIRST_CALLS
    assert list(metrics) == CORE_KEYS + ["candidates", "two_stage", "diversified", "sections", "related", "labels_outside"]
    assert recall == metrics["recall"] and metrics["eval_calls"] == 3 and metrics["sessions"] == 15 and metrics["coverage"] == 17
    lines = [ln.split(" ")[0] for ln in capsys.readouterr().out.splitlines() if not ln.startswith(("batch", "active_", "input_", "Sampler"))]
    assert lines == ["Measuring...", "avg", "avg", "avg", "len", "MRR@20:", "candidates", "two-stage", "diversified", "sections", "related",
                     "labels"]


def test_a_pack_takes_its_diversity_counts_feed_by_feed_and_its_sections_behind_them(fold_and_data, capsys):
    calls, metrics, recall = eval_recorder.recorded_test(Seq2SeqAttNN, *fold_and_data, **PACKED)
    assert calls == PACKED_CALLS
    assert list(metrics) == CORE_KEYS + ["sections", "capped"]
    assert recall == metrics["recall"] and metrics["eval_calls"] == 2 and metrics["sessions"] == 15
    assert [ln.split(" ")[0] for ln in capsys.readouterr().out.splitlines()][-2:] == ["sections", "capped"]


def test_the_plain_loop_makes_one_materialised_call_per_feed_and_no_pass(fold_and_data):
    calls, metrics, _ = eval_recorder.recorded_test(Seq2SeqAttNN, *fold_and_data)
    per_feed = lambda b, t: ['upload B=%d T=%d' % (b, t), 'eval_step B=%d' % b, 'eval_diversity lists=%d block=None' % b]
    assert calls == ['set_categories', 'reset_coverage'] + per_feed(5, 2) + per_feed(2, 1) + per_feed(8, 1) + ['check_forks', 'coverage']
    assert list(metrics) == CORE_KEYS
