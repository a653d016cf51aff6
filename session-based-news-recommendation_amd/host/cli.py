"""Command line of the trainer: the reference's flags (main.py:94-123, same names and defaults) plus the inputs
the reference hard-codes as author paths (main.py:36, util.py:47) and the MI355X-specific switches.

    python main.py --foldnum=0 --epoch=1                      # a fold on disk (data_partition layout)
    python main.py --synthetic 46033 --epoch 1                # synthetic Globo-like fold (no dataset needed)
    python -m torch.distributed.run --nproc-per-node 8 main.py --gpus 8 ...   # data parallel over RCCL

`--save / --is_print / --train` keep argparse `type=bool` (any non-empty string is True), as in the reference.
"""
from __future__ import annotations

import argparse
import os
import pickle
import random
import sys
from typing import NamedTuple, Tuple

import numpy as np

# (flag, default, type, help) — main.py:94-123
REFERENCE_FLAGS = [
    ("datapath", "./data/", str, "Location of pre-processed dataset"),
    ("dataset", "mind/TCAR-mid/", str, "Dataset"),
    ("foldnum", 1, int, "The fold number of pre-processed dataset"),
    ("batch_size", 512, int, "Batch size"),
    ("lr", 0.001, float, "Learning rate"),
    ("epoch", 10, int, "Number of epochs"),
    ("maxlen", 20, int, "Number of max window size"),
    ("neg_num", 20, int, "Number of neg samples"),
    ("model", "model_combine", str, "Model to use"),
    ("hidden_size", 250, int, None),
    ("time_hidden_size", 64, int, None),
    ("max_grad", 150, int, None),
    ("stddev", 0.05, float, None),
    ("emb_stddev", 0.002, float, None),
    ("dropout_rate", 0.5, float, None),
    ("l2_emb", 0.0, float, None),
    ("save", False, bool, "Save model and test results"),
    ("is_print", False, bool, "Save model and test results"),
    ("train", True, bool, "Train or just test the specified model"),
    ("modelpath", "./ckpt/", str, "File to save model checkpoints"),
    ("inputdata", "test", str, "Use train or test data to test model"),
    ("threshold_acc", 0.27, float, "Accuracy threshold to save"),
]


MAX_PANEL = 49152          # the widest panel a fold takes (SEL_MAX_N of csrc/tcar_common.h; engine.TcarEngine.SERVE_MAX_PANEL)


MAX_SECTIONS = 16          # sections of one sectioned call (engine.TcarEngine.MAX_SECTIONS; TCAR_MAX_SECTIONS of include/tcar_sections.h)
MAX_RELATED = 64           # entries of one related-articles list (the k of engine.TcarEngine.similar_items; SEL_MAX_K of csrc/tcar_common.h)
MAX_SHORTLIST = 1024       # entries of one shortlist (engine.TcarEngine.RETRIEVE_MAX_C); a list of up to 64 needs no first stage
MAX_CANDIDATES = 1024      # slots of one candidate list (CAND_MAX_C of csrc/tcar_common.h; engine.TcarEngine.CAND_MAX_C)


class Rule(NamedTuple):
    """One refusal of an evaluation option.  kind and arg say when it applies, text is the refusal, word for word:
      "type" (classes)       the value is a bool or none of `classes`; the only rule that also looks at a value that is off
      "finite"               the value is NaN, infinite or negative
      "range" (lo, hi, step) the value is below lo, above hi or no multiple of step (None: no such bound)
      "engine" which         "one": the option takes ONE engine with the whole catalog, so not --dp_mode sharded;
                             "sharded": it takes the catalog-sharded engine, so only --dp_mode sharded
      "one_process"          more than one data-parallel rank
      "needs" flag           `flag` is off
      "excludes" flag        `flag` is on"""
    kind: str
    arg: object
    text: str


class EvalOption(NamedTuple):
    """One option of the evaluation loop (host/model.py: test()): a command-line flag, a key of the model's args, 0 = off.  `rules`
    holds its accepted range and what it needs and excludes, in the order they are checked."""
    name: str
    type: type
    help: str
    rules: Tuple[Rule, ...]


def _panel_range(flag):
    return Rule("range", (128, MAX_PANEL, 128), "--%s must be a multiple of 128 in [128, %d] (0: off)" % (flag, MAX_PANEL))


def _in(flag, lo, hi):
    return Rule("range", (lo, hi, None), "--%s must be in [%d, %d] (0: off)" % (flag, lo, hi))


def _streamed(flag, what, takes):
    """an option of the streamed evaluation of ONE engine: positive, refused under --dp_mode sharded, and it needs --eval_panel"""
    return (Rule("range", (0, None, None), "--%s must be positive (0: off)" % flag),
            Rule("engine", "one", "--%s %s the streamed evaluation of ONE engine; it cannot be combined with --dp_mode sharded" % (flag, what)),
            Rule("needs", "eval_panel", "--%s needs --eval_panel P: only the streamed evaluation takes a %s" % (flag, takes)))


# In the order check_eval_options walks them: a request that breaks several rules is refused with the first one.
EVAL_OPTIONS = (
    EvalOption("eval_panel", int,
               "P > 0: evaluation scores the catalog P columns at a time and selects while it streams (no [B, N] score matrix, "
               "any catalog size; P % 128 == 0, P <= " + str(MAX_PANEL) + ").  0: the materialised evaluation.  Not with --dp_mode sharded",
               (Rule("engine", "one", "--eval_panel streams the WHOLE catalog through one engine; it cannot be combined with --dp_mode sharded "
                                      "(the catalog-sharded engine evaluates with its own exchange)"),
                _panel_range("eval_panel"))),
    EvalOption("fresh_hours", float,
               "H > 0: evaluation ranks every session inside its POOL — the items published in the H hours up to the label's "
               "click (and the label) — not against the whole catalog.  Needs --eval_panel; not with --dp_mode sharded.  0: off",
               _streamed("fresh_hours", "windows", "publish-time window")),
    EvalOption("cat_cap", int,
               "M > 0: evaluation lists hold at most M items of one category (the walk of include/tcar_quota.h); ILD, unexp and "
               "coverage describe the capped lists, and one more line gives their accuracy.  Needs --eval_panel; not with "
               "--dp_mode sharded; combines with --fresh_hours.  0: off",
               _streamed("cat_cap", "caps", "per-category cap")),
    EvalOption("shard_eval_panel", int,
               "P > 0 (only with --dp_mode sharded): evaluation streams every rank's SHARD of the catalog P columns at a time "
               "and merges the ranks' select states (no [B, N] score matrix on any rank; P % 128 == 0, P <= " + str(MAX_PANEL) + ").  "
               "0: the materialised evaluation of the catalog-sharded engine",
               (_panel_range("shard_eval_panel"),
                Rule("engine", "sharded", "--shard_eval_panel streams the shards of the catalog-sharded engine: it needs --dp_mode sharded "
                                          "(one engine with the whole catalog: --eval_panel)"))),
    EvalOption("eval_sections", int,
               "G > 0: evaluation additionally asks for one list of 20 per CATEGORY on every batch (include/tcar_sections.h: "
               "the G categories with the most catalog items, all from one pass over the catalog) and prints the share of "
               "labels found in the list of their own category; 1 <= G <= " + str(MAX_SECTIONS) + ".  Needs --eval_panel; "
               "combines with --fresh_hours and --eval_mixed; not with --dp_mode sharded.  0: off",
               (Rule("range", (None, MAX_SECTIONS, None), "--eval_sections must be in [1, %d] (0: off)" % MAX_SECTIONS),)
               + _streamed("eval_sections", "lists the categories beside", "list per category")),
    EvalOption("eval_related", int,
               "K > 0: evaluation additionally lists, once behind its batches, the K articles most similar in CONTENT to every "
               "distinct label article of the data (include/tcar_similar.h: the content cosine of the diversity re-rank, the "
               "catalog streamed in panels, no session) and prints their mean cosine and the share that is of the article's own "
               "category; 1 <= K <= " + str(MAX_RELATED) + ".  Not with --dp_mode sharded.  0: off",
               (Rule("type", (int, np.integer), "--eval_related must be an integer in [1, %d] (0: off)" % MAX_RELATED),
                _in("eval_related", 1, MAX_RELATED),
                Rule("engine", "one", "--eval_related reads the content of the WHOLE catalog on one engine; it cannot be combined with "
                                      "--dp_mode sharded"))),
    EvalOption("eval_candidates", int,
               "C > 0: evaluation additionally ranks every label among C - 1 other items drawn uniformly from the catalog "
               "(include/tcar_cand.h: only those C rows are scored) and prints their AUC / MRR / nDCG@5 / nDCG@10; "
               "2 <= C <= " + str(MAX_CANDIDATES) + ".  Not with --dp_mode sharded; combines with everything else.  0: off",
               (_in("eval_candidates", 2, MAX_CANDIDATES),
                Rule("engine", "one", "--eval_candidates scores candidate lists against the WHOLE catalog on one engine; it cannot be "
                                      "combined with --dp_mode sharded"))),
    EvalOption("eval_shortlist", int,
               "C > 0: evaluation additionally runs the two-stage recommendation on every batch (include/tcar_retrieve.h: a "
               "shortlist of C items from coarse scores, re-scored exactly and cut to 20) and prints the share of labels in those "
               "lists and their agreement with the streamed lists; 65 <= C <= " + str(MAX_SHORTLIST) + ".  Needs --eval_panel; "
               "not with --dp_mode sharded, not with --cat_cap.  0: off",
               (_in("eval_shortlist", 65, MAX_SHORTLIST),
                Rule("engine", "one", "--eval_shortlist retrieves from the WHOLE catalog on one engine; it cannot be combined with --dp_mode sharded"),
                Rule("needs", "eval_panel", "--eval_shortlist needs --eval_panel P: its lists are compared with those of the streamed evaluation"),
                Rule("excludes", "cat_cap", "--eval_shortlist cannot be combined with --cat_cap: retrieval takes no per-category cap"))),
    EvalOption("eval_diversity", float,
               "MU > 0: evaluation additionally runs the DIVERSIFIED two-stage recommendation on every batch (include/tcar_mmr.h: "
               "the shortlist's k best under the greedy MMR walk over content, a verbatim duplicate of a listed item losing MU "
               "logits) and prints its Recall@20, ILD and content ILD beside those of the plain two-stage lists.  Needs "
               "--eval_shortlist C; not with --dp_mode sharded.  0: off",
               (Rule("type", (int, float, np.integer, np.floating), "--eval_diversity must be a number (0: off)"),
                Rule("finite", None, "--eval_diversity must be a finite penalty > 0 (0: off)"),
                Rule("engine", "one", "--eval_diversity diversifies the two-stage lists of ONE engine; it cannot be combined with --dp_mode sharded"),
                Rule("needs", "eval_shortlist", "--eval_diversity needs --eval_shortlist C: the walk re-ranks the shortlist of the two-stage call"))),
    EvalOption("shard_eval_shortlist", int,
               "C > 0 (only with --dp_mode sharded and --shard_eval_panel P): evaluation additionally runs the two-stage "
               "recommendation over the shards on every batch (include/tcar_retrieve_shard.h: every shard's shortlist of C items "
               "from coarse scores merged exactly, re-scored by the rows' owners, cut to 20) and prints the line of "
               "--eval_shortlist; 65 <= C <= " + str(MAX_SHORTLIST) + ".  0: off",
               (_in("shard_eval_shortlist", 65, MAX_SHORTLIST),
                Rule("engine", "sharded", "--shard_eval_shortlist merges the shortlists of the catalog-sharded engine: it needs --dp_mode sharded "
                                          "(one engine with the whole catalog: --eval_shortlist)"),
                Rule("needs", "shard_eval_panel", "--shard_eval_shortlist needs --shard_eval_panel P: its lists are compared with those of the "
                                                  "streamed evaluation"))),
    EvalOption("eval_mixed", int,
               "1: evaluation packs consecutive batches of DIFFERENT session lengths into one ragged batch of at most "
               "--batch_size sessions (include/tcar_ragged.h) and streams the catalog once per pack instead of once per batch.  "
               "Needs --eval_panel; combines with --fresh_hours and --cat_cap; not with --dp_mode sharded, --gpus > 1, "
               "--eval_candidates, --eval_shortlist.  0: one call per batch",
               (Rule("range", (0, 1, None), "--eval_mixed must be 0 or 1"),
                Rule("engine", "one", "--eval_mixed packs the streamed evaluation of ONE engine; it cannot be combined with --dp_mode sharded"),
                Rule("one_process", None, "--eval_mixed cannot be combined with --gpus > 1: the ranks split every batch by rows"),
                Rule("needs", "eval_panel", "--eval_mixed needs --eval_panel P: only the streamed evaluation takes a ragged batch"),
                Rule("excludes", "eval_candidates", "--eval_mixed cannot be combined with --eval_candidates"),
                Rule("excludes", "eval_shortlist", "--eval_mixed cannot be combined with --eval_shortlist"))),
)
# where --help lists them (the order the flags were added in)
_HELP_ORDER = ("eval_panel", "fresh_hours", "cat_cap", "shard_eval_panel", "shard_eval_shortlist", "eval_candidates", "eval_shortlist",
               "eval_diversity", "eval_mixed", "eval_sections", "eval_related")
# what Seq2SeqAttNN._eval_request resolves: every option under its name, in its type
EvalRequest = NamedTuple("EvalRequest", [(o.name, o.type) for o in EVAL_OPTIONS])


def check_eval_options(values, gpus=1, options=EVAL_OPTIONS):
    """Refuse a request for the evaluation loop that cannot work: `values` maps dp_mode and any of the options of EVAL_OPTIONS to
    their values (an absent option is off), `gpus` is the number of data-parallel ranks.  The options are walked in the table's
    order, each one's rules in theirs, and the first broken rule is raised as a ValueError.  `options`: another table of the same
    shape (eval_passes.COLD_START_OPTIONS)."""
    sharded = values.get("dp_mode", "replica") == "sharded"
    for opt in options:
        v = values.get(opt.name, 0)
        for kind, arg, text in opt.rules:
            if kind == "type":
                broken = isinstance(v, bool) or not isinstance(v, arg)
            elif not v:
                break                                        # off: nothing else of it to check
            elif kind == "finite":
                broken = v != v or v in (float("inf"), float("-inf")) or v < 0
            elif kind == "range":
                lo, hi, step = arg
                broken = (lo is not None and v < lo) or (hi is not None and v > hi) or (step is not None and v % step)
            elif kind == "engine":
                broken = sharded if arg == "one" else not sharded
            elif kind == "one_process":
                broken = gpus and gpus > 1
            else:
                broken = not values.get(arg) if kind == "needs" else values.get(arg)
            if broken:
                raise ValueError(text)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="TCAR trainer (MI355X-native hot path)")
    for name, default, typ, hlp in REFERENCE_FLAGS:
        ap.add_argument("--" + name, default=default, type=typ, help=hlp)
    ap.add_argument("--split_way", default="Normal/", type=str, choices=["Normal/", "TrainLen/", "TestLen/"],
                    help="Choose different split ways")
    # inputs the reference hard-codes
    ap.add_argument("--category_path", default=None, type=str, help="pickle of article categories (main.py:36)")
    ap.add_argument("--neighbor_path", default=None, type=str, help="pickle of the negative source (util.py:47-48)")
    # call-site toggles the reference leaves as comments (sampler.py:87-99)
    ap.add_argument("--gap_mode", default="active_t", choices=["active_t", "click_delta"])
    ap.add_argument("--neg_mode", default="uniform", choices=["uniform", "neighbor", "impression"])
    ap.add_argument("--device_sampler", default=0, type=int,
                    help="1: training batches are formed and their negatives drawn ON THE GPU from the HBM-resident session store")
    ap.add_argument("--neg_fast", default=0, type=int,
                    help="1: vectorised neighbour / impression negatives (same rules, not the reference's random.choice order)")
    # MI355X
    ap.add_argument("--scoring", default="bf16x3-mixed", choices=["f32", "bf16x3", "bf16x3-mixed", "bf16"],
                    help="precision of the full-catalog scoring GEMMs (bf16x3-mixed = what bench.py measures: logits on split-bf16 planes, "
                         "fp32-class; the two gradient GEMMs on plain bf16 operands.  bf16x3: all three fp32-class)")
    ap.add_argument("--gpus", default=1, type=int, help="data-parallel ranks (launch with torch.distributed.run)")
    ap.add_argument("--dp_mode", default="replica", choices=["replica", "sharded"],
                    help="multi-GPU exchange: replica = all-reduce of the dense item gradient (dp.py); sharded = catalog-sharded "
                         "scoring (sharded.py: the item gradient stays on the rank that owns the rows)")
    by_name = {o.name: o for o in EVAL_OPTIONS}
    for name in _HELP_ORDER:                                 # every evaluation option defaults to 0: off
        ap.add_argument("--" + name, default=0, type=by_name[name].type, help=by_name[name].help)
    from .eval_passes import COLD_START_FLAGS, COLD_START_OPTIONS, DEFAULT_DONORS      # (here: eval_passes builds on this module)
    for flag, opt in zip(COLD_START_FLAGS, COLD_START_OPTIONS):
        ap.add_argument("--" + flag, dest=opt.name, default=DEFAULT_DONORS if opt.name == "coldstart_donors" else 0, type=opt.type,
                        help=opt.help)
    ap.add_argument("--audit_duplicates", default=0.0, type=float,
                    help="T in (0, 1]: behind training or testing, audit the WHOLE catalog for near-duplicate articles "
                         "(include/tcar_dupes.h: every pair of content rows once, cosine >= T) and print how many articles fall into "
                         "how many groups.  Not an evaluation option; not with --dp_mode sharded or --gpus > 1.  0: off")
    ap.add_argument("--synthetic", default=0, type=int, help="N items of a synthetic Globo-like fold (no files)")
    ap.add_argument("--synthetic_train", default=100000, type=int)
    ap.add_argument("--synthetic_test", default=10000, type=int)
    ap.add_argument("--seed", default=2020, type=int)
    return ap


def check_audit_option(threshold, dp_mode="replica", gpus=1):
    """Refuse an --audit_duplicates that cannot work, before any data is loaded (0: off, nothing to check)"""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or threshold != threshold \
            or not 0 <= threshold <= 1:
        raise ValueError("--audit_duplicates must be a cosine threshold in (0, 1] (0: off)")
    if threshold and dp_mode == "sharded":
        raise ValueError("--audit_duplicates pairs every article with every other on ONE engine with the whole catalog; it cannot be "
                         "combined with --dp_mode sharded")
    if threshold and gpus and gpus > 1:
        raise ValueError("--audit_duplicates cannot be combined with --gpus > 1: one engine audits the catalog")


def audit_duplicates(model, threshold):
    """the audit behind --audit_duplicates: one line, and what it was computed from -> (groups, audit)"""
    import torch
    groups, audit = model.duplicate_articles(threshold=threshold)
    pairs = int(audit.count.sum(dtype=torch.int64).item()) // 2             # every pair counts once at each of its two articles
    print("duplicate audit (cosine >= {}): {} articles in {} groups, largest {}, {} pairs".format(
        threshold, sum(len(g) for g in groups), len(groups), max((len(g) for g in groups), default=0), pairs))
    return groups, audit


def load_datas(args):
    """main.py:14-47: returns train_data, test_data, neighbor, args(dict), item_dict."""
    print("load the datasets.")
    a = vars(args).copy()
    if args.synthetic:
        from .synth import SynthFold
        fold = SynthFold(n_items=args.synthetic, dim=args.hidden_size, n_train=args.synthetic_train,
                         n_test=args.synthetic_test, seed=args.seed, active_t=(args.gap_mode == "active_t"))

        def as_data(store):
            len_dict = {}
            for T in np.unique(store.in_len):
                len_dict[int(T)] = np.where(store.in_len == T)[0].tolist()
            return (len_dict, None, None, store)

        train_data, test_data = as_data(fold.train), as_data(fold.test)
        item_dict = fold.item_dict
        if args.neg_mode == "neighbor":
            neighbor = fold.neighbor_dict()
        elif args.neg_mode == "impression":
            neighbor = fold.impression_dict(fold.train)
        else:
            neighbor = {0: [0]}                                                          # truthy => negatives on
        a.update(fold.model_args())
        for k, v in vars(args).items():
            a[k] = v
    else:
        from .data import load_fold
        base = args.datapath + args.dataset + args.split_way
        train_data, test_data, item_dict, neighbor, content_emb, publish_time, _ = load_fold(
            base, args.foldnum, args.neighbor_path)
        if args.neg_mode == "neighbor" and not neighbor:
            # no neighbor_<fold>.txt next to the fold and no --neighbor_path: build it as generate_neighbor.py does
            from .data import build_neighbor
            neighbor = build_neighbor(publish_time[0])
        freq = base + 'item_freq_dict_norm_' + str(args.foldnum) + '.txt'
        a['item_freq_dict_norm'] = pickle.load(open(freq, 'rb')) if os.path.exists(freq) else None
        a['reverse_item'] = {cnt - 1: idx for idx, cnt in item_dict.items()}
        if args.category_path:
            a['category_id'] = pickle.load(open(args.category_path, 'rb'))
        else:
            a['category_id'] = {idx: 0 for idx in item_dict}     # no category file: ILD / unexp degenerate to 0
        a['publish_time'] = publish_time[0]
        a['publish_time_MWDHM'] = publish_time[1]
        a['content_emb'] = content_emb
    a["itemnum"] = len(item_dict)
    print('------', len(item_dict), len(a['publish_time_MWDHM']))
    return train_data, test_data, neighbor, a, item_dict


def main(argv=None):
    args = build_parser().parse_args(argv)
    random.seed(args.seed)                       # main.py:10-12
    np.random.seed(args.seed)
    is_train, model_path, input_data = args.train, args.modelpath, args.inputdata
    check_eval_options(vars(args), args.gpus)
    check_audit_option(args.audit_duplicates, args.dp_mode, args.gpus)
    from .eval_passes import check_cold_start_options
    check_cold_start_options(vars(args), args.gpus)
    dp_group = None
    if args.gpus > 1:
        import torch
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        local = int(os.environ.get("LOCAL_RANK", "0"))
        backend = os.environ.get("TCAR_DIST_BACKEND", "nccl")       # "gloo" + TCAR_SAME_DEVICE=1: dry runs on one GPU
        if os.environ.get("TCAR_SAME_DEVICE"):
            local = 0
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda:%d" % local))
        else:
            dist.init_process_group(backend)
        dp_group = dist.group.WORLD
    train_data, test_data, neighbor, a, item_dict = load_datas(args)
    if dp_group is not None:
        import torch
        a['dp_group'] = dp_group
        a['device'] = "cuda:%d" % torch.cuda.current_device()
    modname = args.model
    mod = __import__(modname, fromlist=True)     # main.py:65-66 plug-in protocol
    model = getattr(mod, "Seq2SeqAttNN")(a)
    if is_train:
        print('Begin Training')
        # The reference never forwards --threshold_acc (main.py:76: train() keeps its default 0.99, so nothing is ever
        # saved).  Here `--save 1` makes the flag live; without it the reference's behaviour is kept.
        if args.save:
            model.train(None, item_dict, train_data, neighbor, a, test_data, None, threshold_acc=args.threshold_acc)
        else:
            model.train(None, item_dict, train_data, neighbor, a, test_data, None)
        if getattr(model, "train_seconds", None):
            print("[tcar] last epoch: %d sessions in %.2f s = %.0f sessions/s (host sampler + H2D + device step)"
                  % (model.train_sessions, model.train_seconds, model.train_sessions / model.train_seconds),
                  file=sys.stderr)
    else:
        import torch
        sent = train_data if input_data == "train" else test_data
        print('Begin Testing. Test data is %s data' % ("train" if input_data == "train" else "test"))
        with np.load(model_path, allow_pickle=False) as ck:          # plain arrays only: nothing is unpickled
            model.engine.load_state(ck)
        model.test(None, sent, a)
    if args.audit_duplicates:
        audit_duplicates(model, args.audit_duplicates)
    if dp_group is not None:
        import torch.distributed as dist
        model.engine.close()                     # the direct RCCL communicator, before the group it was built through
        dist.destroy_process_group()
    return model


if __name__ == "__main__":
    main(sys.argv[1:])
