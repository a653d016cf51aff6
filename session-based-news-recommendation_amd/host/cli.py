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
    ap.add_argument("--eval_panel", default=0, type=int,
                    help="P > 0: evaluation scores the catalog P columns at a time and selects while it streams (no [B, N] score matrix, "
                         "any catalog size; P % 128 == 0, P <= " + str(MAX_PANEL) + ").  0: the materialised evaluation.  Not with --dp_mode sharded")
    ap.add_argument("--fresh_hours", default=0, type=float,
                    help="H > 0: evaluation ranks every session inside its POOL — the items published in the H hours up to the label's "
                         "click (and the label) — not against the whole catalog.  Needs --eval_panel; not with --dp_mode sharded.  0: off")
    ap.add_argument("--cat_cap", default=0, type=int,
                    help="M > 0: evaluation lists hold at most M items of one category (the walk of include/tcar_quota.h); ILD, unexp and "
                         "coverage describe the capped lists, and one more line gives their accuracy.  Needs --eval_panel; not with "
                         "--dp_mode sharded; combines with --fresh_hours.  0: off")
    ap.add_argument("--shard_eval_panel", default=0, type=int,
                    help="P > 0 (only with --dp_mode sharded): evaluation streams every rank's SHARD of the catalog P columns at a time "
                         "and merges the ranks' select states (no [B, N] score matrix on any rank; P % 128 == 0, P <= " + str(MAX_PANEL) + ").  "
                         "0: the materialised evaluation of the catalog-sharded engine")
    ap.add_argument("--shard_eval_shortlist", default=0, type=int,
                    help="C > 0 (only with --dp_mode sharded and --shard_eval_panel P): evaluation additionally runs the two-stage "
                         "recommendation over the shards on every batch (include/tcar_retrieve_shard.h: every shard's shortlist of C items "
                         "from coarse scores merged exactly, re-scored by the rows' owners, cut to 20) and prints the line of "
                         "--eval_shortlist; 65 <= C <= " + str(MAX_SHORTLIST) + ".  0: off")
    ap.add_argument("--eval_candidates", default=0, type=int,
                    help="C > 0: evaluation additionally ranks every label among C - 1 other items drawn uniformly from the catalog "
                         "(include/tcar_cand.h: only those C rows are scored) and prints their AUC / MRR / nDCG@5 / nDCG@10; "
                         "2 <= C <= " + str(MAX_CANDIDATES) + ".  Not with --dp_mode sharded; combines with everything else.  0: off")
    ap.add_argument("--eval_shortlist", default=0, type=int,
                    help="C > 0: evaluation additionally runs the two-stage recommendation on every batch (include/tcar_retrieve.h: a "
                         "shortlist of C items from coarse scores, re-scored exactly and cut to 20) and prints the share of labels in those "
                         "lists and their agreement with the streamed lists; 65 <= C <= " + str(MAX_SHORTLIST) + ".  Needs --eval_panel; "
                         "not with --dp_mode sharded, not with --cat_cap.  0: off")
    ap.add_argument("--eval_diversity", default=0, type=float,
                    help="MU > 0: evaluation additionally runs the DIVERSIFIED two-stage recommendation on every batch (include/tcar_mmr.h: "
                         "the shortlist's k best under the greedy MMR walk over content, a verbatim duplicate of a listed item losing MU "
                         "logits) and prints its Recall@20, ILD and content ILD beside those of the plain two-stage lists.  Needs "
                         "--eval_shortlist C; not with --dp_mode sharded.  0: off")
    ap.add_argument("--eval_mixed", default=0, type=int,
                    help="1: evaluation packs consecutive batches of DIFFERENT session lengths into one ragged batch of at most "
                         "--batch_size sessions (include/tcar_ragged.h) and streams the catalog once per pack instead of once per batch.  "
                         "Needs --eval_panel; combines with --fresh_hours and --cat_cap; not with --dp_mode sharded, --gpus > 1, "
                         "--eval_candidates, --eval_shortlist.  0: one call per batch")
    ap.add_argument("--eval_sections", default=0, type=int,
                    help="G > 0: evaluation additionally asks for one list of 20 per CATEGORY on every batch (include/tcar_sections.h: "
                         "the G categories with the most catalog items, all from one pass over the catalog) and prints the share of "
                         "labels found in the list of their own category; 1 <= G <= " + str(MAX_SECTIONS) + ".  Needs --eval_panel; "
                         "combines with --fresh_hours and --eval_mixed; not with --dp_mode sharded.  0: off")
    ap.add_argument("--eval_related", default=0, type=int,
                    help="K > 0: evaluation additionally lists, once behind its batches, the K articles most similar in CONTENT to every "
                         "distinct label article of the data (include/tcar_similar.h: the content cosine of the diversity re-rank, the "
                         "catalog streamed in panels, no session) and prints their mean cosine and the share that is of the article's own "
                         "category; 1 <= K <= " + str(MAX_RELATED) + ".  Not with --dp_mode sharded.  0: off")
    ap.add_argument("--synthetic", default=0, type=int, help="N items of a synthetic Globo-like fold (no files)")
    ap.add_argument("--synthetic_train", default=100000, type=int)
    ap.add_argument("--synthetic_test", default=10000, type=int)
    ap.add_argument("--seed", default=2020, type=int)
    return ap


def _check_panel(flag, panel):
    if panel < 0 or panel % 128 or panel > MAX_PANEL:
        raise ValueError("--%s must be a multiple of 128 in [128, %d] (0: off)" % (flag, MAX_PANEL))


def _check_streamed_option(flag, value, what, takes, eval_panel, dp_mode):
    """an option of the streamed evaluation of ONE engine: positive, refused under --dp_mode sharded, and it needs --eval_panel"""
    if not value:
        return
    if value < 0:
        raise ValueError("--%s must be positive (0: off)" % flag)
    if dp_mode == "sharded":
        raise ValueError("--%s %s the streamed evaluation of ONE engine; it cannot be combined with --dp_mode sharded" % (flag, what))
    if not eval_panel:
        raise ValueError("--%s needs --eval_panel P: only the streamed evaluation takes a %s" % (flag, takes))


def check_eval_panel(eval_panel, dp_mode):
    """--eval_panel is the single-engine streamed evaluation: the catalog-sharded engine keeps its own evaluation"""
    if eval_panel and dp_mode == "sharded":
        raise ValueError("--eval_panel streams the WHOLE catalog through one engine; it cannot be combined with --dp_mode sharded "
                         "(the catalog-sharded engine evaluates with its own exchange)")
    _check_panel("eval_panel", eval_panel)


def check_fresh_hours(fresh_hours, eval_panel, dp_mode):
    """--fresh_hours windows the streamed evaluation (include/tcar_window.h): it needs --eval_panel and the whole catalog on one engine"""
    _check_streamed_option("fresh_hours", fresh_hours, "windows", "publish-time window", eval_panel, dp_mode)


def check_cat_cap(cat_cap, eval_panel, dp_mode):
    """--cat_cap caps the lists of the streamed evaluation (include/tcar_quota.h): it needs --eval_panel and the whole catalog on one engine"""
    _check_streamed_option("cat_cap", cat_cap, "caps", "per-category cap", eval_panel, dp_mode)


def check_eval_sections(eval_sections, eval_panel, dp_mode):
    """--eval_sections asks one engine for a list per category beside its streamed evaluation (include/tcar_sections.h): it needs
    --eval_panel and the whole catalog on one engine"""
    if eval_sections > MAX_SECTIONS:
        raise ValueError("--eval_sections must be in [1, %d] (0: off)" % MAX_SECTIONS)
    _check_streamed_option("eval_sections", eval_sections, "lists the categories beside", "list per category", eval_panel, dp_mode)


def check_eval_related(eval_related, dp_mode):
    """--eval_related lists the articles related to every label article (include/tcar_similar.h), which takes the whole catalog on
    one engine"""
    if isinstance(eval_related, bool) or not isinstance(eval_related, (int, np.integer)):
        raise ValueError("--eval_related must be an integer in [1, %d] (0: off)" % MAX_RELATED)
    if not eval_related:
        return
    if eval_related < 1 or eval_related > MAX_RELATED:
        raise ValueError("--eval_related must be in [1, %d] (0: off)" % MAX_RELATED)
    if dp_mode == "sharded":
        raise ValueError("--eval_related reads the content of the WHOLE catalog on one engine; it cannot be combined with "
                         "--dp_mode sharded")


def check_shard_eval_panel(shard_eval_panel, dp_mode):
    """--shard_eval_panel is the streamed evaluation of the catalog-sharded engine (include/tcar_serve_shard.h)"""
    _check_panel("shard_eval_panel", shard_eval_panel)
    if shard_eval_panel and dp_mode != "sharded":
        raise ValueError("--shard_eval_panel streams the shards of the catalog-sharded engine: it needs --dp_mode sharded "
                         "(one engine with the whole catalog: --eval_panel)")


def check_eval_candidates(eval_candidates, dp_mode):
    """--eval_candidates ranks the label among sampled items through candidate-list scoring (include/tcar_cand.h), which takes the
    whole catalog on one engine"""
    if not eval_candidates:
        return
    if eval_candidates < 2 or eval_candidates > MAX_CANDIDATES:
        raise ValueError("--eval_candidates must be in [2, %d] (0: off)" % MAX_CANDIDATES)
    if dp_mode == "sharded":
        raise ValueError("--eval_candidates scores candidate lists against the WHOLE catalog on one engine; it cannot be combined with "
                         "--dp_mode sharded")


def check_eval_shortlist(eval_shortlist, eval_panel, dp_mode, cat_cap=0):
    """--eval_shortlist runs the two-stage recommendation (include/tcar_retrieve.h) beside the streamed evaluation of ONE engine and
    compares their lists: it needs --eval_panel and the whole catalog on one engine, and retrieval takes no per-category cap"""
    if not eval_shortlist:
        return
    if eval_shortlist < 65 or eval_shortlist > MAX_SHORTLIST:
        raise ValueError("--eval_shortlist must be in [65, %d] (0: off)" % MAX_SHORTLIST)
    if dp_mode == "sharded":
        raise ValueError("--eval_shortlist retrieves from the WHOLE catalog on one engine; it cannot be combined with --dp_mode sharded")
    if not eval_panel:
        raise ValueError("--eval_shortlist needs --eval_panel P: its lists are compared with those of the streamed evaluation")
    if cat_cap:
        raise ValueError("--eval_shortlist cannot be combined with --cat_cap: retrieval takes no per-category cap")


def check_eval_diversity(eval_diversity, eval_shortlist, dp_mode):
    """--eval_diversity runs the diversified two-stage recommendation (include/tcar_mmr.h) beside the plain one: a finite penalty
    MU > 0 in score units, the shortlist of --eval_shortlist, and the whole catalog on one engine"""
    if isinstance(eval_diversity, bool) or not isinstance(eval_diversity, (int, float, np.integer, np.floating)):
        raise ValueError("--eval_diversity must be a number (0: off)")
    if eval_diversity != eval_diversity or eval_diversity in (float("inf"), float("-inf")) or eval_diversity < 0:
        raise ValueError("--eval_diversity must be a finite penalty > 0 (0: off)")
    if not eval_diversity:
        return
    if dp_mode == "sharded":
        raise ValueError("--eval_diversity diversifies the two-stage lists of ONE engine; it cannot be combined with --dp_mode sharded")
    if not eval_shortlist:
        raise ValueError("--eval_diversity needs --eval_shortlist C: the walk re-ranks the shortlist of the two-stage call")


def check_shard_eval_shortlist(shard_eval_shortlist, shard_eval_panel, dp_mode):
    """--shard_eval_shortlist runs the two-stage recommendation of the catalog-sharded engine (include/tcar_retrieve_shard.h) beside
    its streamed evaluation and compares their lists: it needs --dp_mode sharded and --shard_eval_panel"""
    if not shard_eval_shortlist:
        return
    if shard_eval_shortlist < 65 or shard_eval_shortlist > MAX_SHORTLIST:
        raise ValueError("--shard_eval_shortlist must be in [65, %d] (0: off)" % MAX_SHORTLIST)
    if dp_mode != "sharded":
        raise ValueError("--shard_eval_shortlist merges the shortlists of the catalog-sharded engine: it needs --dp_mode sharded "
                         "(one engine with the whole catalog: --eval_shortlist)")
    if not shard_eval_panel:
        raise ValueError("--shard_eval_shortlist needs --shard_eval_panel P: its lists are compared with those of the streamed evaluation")


def check_eval_mixed(eval_mixed, eval_panel, dp_mode, gpus=1, eval_candidates=0, eval_shortlist=0):
    """--eval_mixed packs the batches of the streamed evaluation of ONE engine into ragged batches (include/tcar_ragged.h): it needs
    --eval_panel and one process; the candidate and two-stage passes keep their rectangular batches"""
    if not eval_mixed:
        return
    if eval_mixed not in (0, 1):
        raise ValueError("--eval_mixed must be 0 or 1")
    if dp_mode == "sharded":
        raise ValueError("--eval_mixed packs the streamed evaluation of ONE engine; it cannot be combined with --dp_mode sharded")
    if gpus and gpus > 1:
        raise ValueError("--eval_mixed cannot be combined with --gpus > 1: the ranks split every batch by rows")
    if not eval_panel:
        raise ValueError("--eval_mixed needs --eval_panel P: only the streamed evaluation takes a ragged batch")
    if eval_candidates:
        raise ValueError("--eval_mixed cannot be combined with --eval_candidates")
    if eval_shortlist:
        raise ValueError("--eval_mixed cannot be combined with --eval_shortlist")


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
    check_eval_panel(args.eval_panel, args.dp_mode)
    check_fresh_hours(args.fresh_hours, args.eval_panel, args.dp_mode)
    check_cat_cap(args.cat_cap, args.eval_panel, args.dp_mode)
    check_shard_eval_panel(args.shard_eval_panel, args.dp_mode)
    check_eval_sections(args.eval_sections, args.eval_panel, args.dp_mode)
    check_eval_related(args.eval_related, args.dp_mode)
    check_eval_candidates(args.eval_candidates, args.dp_mode)
    check_eval_shortlist(args.eval_shortlist, args.eval_panel, args.dp_mode, args.cat_cap)
    check_eval_diversity(args.eval_diversity, args.eval_shortlist, args.dp_mode)
    check_shard_eval_shortlist(args.shard_eval_shortlist, args.shard_eval_panel, args.dp_mode)
    check_eval_mixed(args.eval_mixed, args.eval_panel, args.dp_mode, args.gpus, args.eval_candidates, args.eval_shortlist)
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
    if dp_group is not None:
        import torch.distributed as dist
        model.engine.close()                     # the direct RCCL communicator, before the group it was built through
        dist.destroy_process_group()
    return model


if __name__ == "__main__":
    main(sys.argv[1:])
