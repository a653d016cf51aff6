"""The optional measurements of `Seq2SeqAttNN.test()`, one class each, with the same three moments:

  * construction from the model and the resolved request (cli.EvalRequest) — only for a pass that is on;
  * `after_feed(feeds, bt, topk, window, rows_cap)`, once per streamed call, behind the loop's own diversity counts: the feeds of
    that call (one; several under eval_mixed, packed into one ragged batch), their uploaded batch, the streamed lists — the step's
    own buffer: whoever keeps it clones it —, the (lo, hi) of fresh_hours or None, the capacity of this rank's shard or None.  It
    issues the pass's engine calls and keeps CLONED device results: no copy to the host, no synchronisation before check_forks();
  * `report(n, results)`, behind check_forks() and the core metrics: it drains what it kept, sums over the ranks (model._allsum, a
    collective: every rank reports every active pass), prints its line and returns the pass's entry of `last_metrics`.  n: the
    sessions of all ranks; results: the loop's FeedResult per feed of this rank.

`active_passes` lists them in the ONE order that is the order of their engine calls behind a streamed call, of their lines and of
their collectives.  The classes say where a shared workspace of the engine fixes that order.

A pass that WRITES the engine (ColdStart) declares its options here, in COLD_START_OPTIONS — rows of the same shape as
cli.EVAL_OPTIONS, walked by the same cli.check_eval_options —, beside the pass they switch on.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import cli, metrics as M
from .cli import EvalOption, Rule
from .data import pack_sessions


class FeedResult(NamedTuple):
    """what test() keeps of one feed until its drain: the feed and CLONES of its device results.  topk is kept only for is_print
    and cat_cap (nothing else reads the streamed lists after the loop)."""
    feed: dict
    rank: torch.Tensor
    topk: Optional[torch.Tensor]
    ce: torch.Tensor
    ild_c: torch.Tensor
    unexp_c: torch.Tensor
    n_rec: torch.Tensor


def _sessions(feed):
    """a feed as the serving calls take it: no label, no negatives"""
    return {n: v for n, v in feed.items() if n not in ("label", "neg")}


def _labels(feeds):
    return np.concatenate([np.asarray(f["label"], dtype=np.int64).reshape(-1) for f in feeds])


class EvalPass:
    key = None                                   # the pass's entry of last_metrics

    def __init__(self, model, req):
        self.m, self.eng, self.req, self.kept = model, model.engine, req, []

    def after_feed(self, feeds, bt, topk, window, rows_cap):
        pass

    def idle(self, rows_cap, T):
        """data parallel: this rank's shard of a feed is empty.  A pass whose engine calls are collectives joins them here."""


class Candidates(EvalPass):
    """eval_candidates C: every label among C - 1 items sampled from the catalog (include/tcar_cand.h: only those rows are scored).
    The lists are drawn from a RandomState(seed) of the pass's own, so no other random stream of the run moves."""
    key = "candidates"

    def __init__(self, model, req):
        super().__init__(model, req)
        self.rng = np.random.RandomState(model.seed)

    def after_feed(self, feeds, bt, topk, window, rows_cap):
        res = self.eng.score_candidates(None, *self.m._label_among_sampled(feeds[0]["label"], self.req.eval_candidates, self.rng), bt=bt)
        self.kept.append((res.counts.clone(), res.metrics.clone()))

    def report(self, n, results):
        per = [M.impression_metrics(c.cpu().numpy(), m.cpu().numpy()) for c, m in self.kept]
        cols = [np.concatenate([p[i] for p in per]) if per else np.zeros(0) for i in range(4)]
        keep = ~np.isnan(cols[0])                # (a label and its negatives always hold both classes; kept for the rule's sake)
        tot = self.m._allsum([float(np.sum(x[keep])) for x in cols] + [float(keep.sum())])
        c_auc, c_mrr, c_n5, c_n10 = [v / max(tot[4], 1.0) for v in tot[:4]]
        print('candidates ({} per session): AUC: {}, MRR: {}, nDCG@5: {}, nDCG@10: {}'.format(self.req.eval_candidates, c_auc, c_mrr, c_n5, c_n10))
        return {"auc": c_auc, "mrr": c_mrr, "ndcg5": c_n5, "ndcg10": c_n10}


class TwoStage(EvalPass):
    """eval_shortlist C (include/tcar_retrieve.h) or, on the catalog-sharded engine, shard_eval_shortlist C
    (include/tcar_retrieve_shard.h): the two-stage lists of the same sessions beside the streamed ones — one line, the same metrics.
    The sharded call is a COLLECTIVE: a rank without sessions still joins it (`idle`), and because the sharded calls share the
    gathered-row workspace the streamed lists are cloned before it.  `kept` holds (labels, streamed lists, two-stage lists), all
    clones: Diversified reads the last entry."""
    key = "two_stage"

    def __init__(self, model, req):
        super().__init__(model, req)
        self.sharded = req.shard_eval_shortlist
        self.shortlist = req.eval_shortlist or self.sharded

    def after_feed(self, feeds, bt, topk, window, rows_cap):
        feed = feeds[0]
        if self.sharded:
            topk = topk.clone()
            two, _ = self.eng.shard_recommend_two_stage(_sessions(feed), k=20, shortlist=self.sharded, exclude_seen=False,
                                                        panel=self.req.shard_eval_panel, window=window, cap=rows_cap)
            self.kept.append((feed["label"], topk, two.clone()))
        else:
            two, _ = self.eng.recommend_two_stage(_sessions(feed), k=20, shortlist=self.shortlist, exclude_seen=False,
                                                  panel=self.req.eval_panel, window=window)
            two = two.clone()
            self.kept.append((feed["label"], topk.clone(), two))

    def idle(self, rows_cap, T):
        if self.sharded:
            self.eng.shard_recommend_two_stage(None, k=20, shortlist=self.sharded, exclude_seen=False, panel=self.req.shard_eval_panel,
                                               cap=rows_cap, T=T)

    def report(self, n, results):
        inside, agree = [], []
        for label, streamed, two in self.kept:
            two, streamed = two.cpu().numpy(), streamed.cpu().numpy()
            inside += (two == np.asarray(label)[:, None]).any(1).tolist()
            agree += [len(set(t[t >= 0].tolist()) & set(s_.tolist())) / 20.0 for t, s_ in zip(two, streamed)]
        t_hit, t_agree = [v / n for v in self.m._allsum([float(np.sum(inside)), float(np.sum(agree))])]
        print('two-stage lists (shortlist {}): Recall@20: {}, agreement with the streamed lists: {}'.format(self.shortlist, t_hit, t_agree))
        return {"recall": t_hit, "agreement": t_agree, "shortlist": self.shortlist}


class Diversified(EvalPass):
    """eval_diversity MU (include/tcar_mmr.h): the diversified form of the plain two-stage lists — the same shortlist, the MMR walk
    over content as its close.  It runs directly behind TwoStage, whose call wrote the workspace this one overwrites, and compares
    with the clone TwoStage kept of the same feed's lists.  Not on the catalog-sharded engine."""
    key = "diversified"

    def __init__(self, model, req, two_stage):
        super().__init__(model, req)
        self.two_stage = two_stage

    def after_feed(self, feeds, bt, topk, window, rows_cap):
        label, _, two = self.two_stage.kept[-1]
        div, _ = self.eng.recommend_two_stage(_sessions(feeds[0]), k=20, shortlist=self.two_stage.shortlist, exclude_seen=False,
                                              panel=self.req.eval_panel, window=window, diversity=self.req.eval_diversity)
        self.kept.append((label, two, div.clone()))

    def report(self, n, results):
        cat, content = self.m._category_table(), np.asarray(self.eng._content)[1:]

        def list_means(lists):
            """sums over the sessions whose list is full (category ILD divides by k (k - 1), as getILD does) -> their count too"""
            full = lists[(lists >= 0).all(1)]
            return [float(M.ild_batch(full, cat).sum()), float(M.content_ild_batch(full, content).sum()), float(len(full))]
        tot = np.zeros(7)
        for label, two, div in self.kept:
            two, div = two.cpu().numpy(), div.cpu().numpy()
            tot += [float((div == np.asarray(label)[:, None]).any(1).sum())] + list_means(div) + list_means(two)
        tot = self.m._allsum(tot.tolist())
        d_hit, d_ild, d_cild = tot[0] / n, tot[1] / max(tot[3], 1.0), tot[2] / max(tot[3], 1.0)
        t_ild, t_cild = tot[4] / max(tot[6], 1.0), tot[5] / max(tot[6], 1.0)
        short, mu = self.two_stage.shortlist, self.req.eval_diversity
        print('diversified lists (shortlist {}, penalty {}): Recall@20: {}, ILD: {}, content ILD: {} (two-stage lists: ILD {}, '
              'content ILD {})'.format(short, mu, d_hit, d_ild, d_cild, t_ild, t_cild))
        return {"recall": d_hit, "ild": d_ild, "content_ild": d_cild, "two_stage_ild": t_ild, "two_stage_content_ild": t_cild,
                "shortlist": short, "penalty": mu}


class Sections(EvalPass):
    """eval_sections G (include/tcar_sections.h): one list of 20 per category for the sessions of the streamed call — the feeds of a
    pack in one ragged call — the sections being the G categories with the most catalog items.  The call uploads the feeds again,
    so it is the last engine call behind a streamed call: behind the diversity counts of the whole pack and behind every other pass."""
    key = "sections"

    def __init__(self, model, req):
        super().__init__(model, req)
        self.sections = M.largest_categories(model._category_table(), req.eval_sections)

    def after_feed(self, feeds, bt, topk, window, rows_cap):
        bare = [_sessions(f) for f in feeds]
        res = self.eng.recommend_sections(bare[0] if len(bare) == 1 else pack_sessions(bare), self.sections, k=20, exclude_seen=False,
                                          panel=self.req.eval_panel, window=window)
        self.kept.append((np.concatenate([np.asarray(f["label"]).reshape(-1) for f in feeds]), res.topk.clone()))

    def report(self, n, results):
        cat = self.m._category_table()
        hc = [M.section_hits(tk.cpu().numpy(), lab, cat, self.sections) for lab, tk in self.kept]
        s_hit, s_cov = self.m._allsum([float(sum(h.sum() for h, _ in hc)), float(sum(c.sum() for _, c in hc))])
        s_recall, s_share = s_hit / max(s_cov, 1.0), s_cov / n
        print('sections ({} categories, 20 per section): Recall@20 in the label\'s section: {}, labels in a listed section: {}'.format(
            len(self.sections), s_recall, s_share))
        return {"G": int(len(self.sections)), "recall": s_recall, "covered": s_share}


class Related(EvalPass):
    """eval_related K (include/tcar_similar.h): the K related articles of every distinct label article of THIS rank's feeds, listed
    once behind the batches — its engine calls are in `report`, batch_size queries a call; the sums go over the ranks."""
    key = "related"

    def report(self, n, results):
        cat, step, k = self.m._category_table(), max(int(self.m.batch_size), 1), self.req.eval_related
        arts = np.unique(_labels([r.feed for r in results])) if results else np.zeros(0, np.int64)
        tot = np.zeros(4)
        for i in range(0, len(arts), step):
            ids = arts[i:i + step]
            tk, sims = (t.cpu().numpy() for t in self.eng.similar_items(ids, k=k))
            cos, same = M.related_sums(tk, sims, ids, cat)
            tot += [cos, same, float((tk >= 0).sum()), float(len(ids))]
        tot = self.m._allsum(tot.tolist())
        r_cos, r_same = tot[0] / max(tot[2], 1.0), tot[1] / max(tot[2], 1.0)
        print('related articles ({} per article): mean cosine: {}, same category: {}'.format(k, r_cos, r_same))
        return {"k": k, "mean_cosine": r_cos, "same_category": r_same, "articles": int(tot[3])}


class LabelsOutside(EvalPass):
    """fresh_hours H: the share of labels published outside their session's window.  (These labels are still scored: a label is
    always in its session's pool.)  Host work only."""
    key = "labels_outside"

    def after_feed(self, feeds, bt, topk, window, rows_cap):
        lo, hi = window
        kl = self.m._item_keys()[_labels(feeds)].astype(np.int64)
        self.kept += (~((lo <= kl) & (kl < hi))).tolist()

    def report(self, n, results):
        share = self.m._allsum([float(np.sum(self.kept))])[0] / n
        print('labels outside their window: {}'.format(share))
        return share


class Capped(EvalPass):
    """cat_cap M: the accuracy of the capped LISTS — the label's place in its list, read from the streamed lists that the loop
    kept (FeedResult.topk); the core metrics' rank is that of the whole pool."""
    key = "capped"

    def report(self, n, results):
        hits, mrrs, ndcgs = [], [], []
        for r in results:
            for col, x in zip((hits, mrrs, ndcgs), M.metrics_from_ranks(M.list_ranks(r.topk.cpu().numpy(), r.feed["label"], 20), 20)):
                col += x.tolist()
        c_mrr, c_hit, c_ndcg = [v / n for v in self.m._allsum([float(np.sum(x)) for x in (mrrs, hits, ndcgs)])]
        print('capped lists (<= {} per category): MRR@20: {}, Recall@20: {}, nDCG@20: {}'.format(self.req.cat_cap, c_mrr, c_hit, c_ndcg))
        return {"mrr": c_mrr, "recall": c_hit, "ndcg": c_ndcg}


MAX_DONORS = 64            # donors of one warm-started row (the k of engine.TcarEngine.warm_start_items; SEL_MAX_K of csrc/tcar_common.h)
DEFAULT_DONORS = 16

# (name: the key of the model's args and the dest of the flag; the flags are COLD_START_FLAGS, in this order)
COLD_START_OPTIONS = (
    EvalOption("coldstart", float,
               "FRAC in (0, 0.5]: behind its batches, evaluation draws a FRAC sample of the distinct label articles of the data "
               "(a random stream of its own: a function of --seed alone) and evaluates the sessions whose label is in the sample "
               "three ways — with the trained item rows, with those rows zeroed, and with those rows written by "
               "warm_start_items (include/tcar_warm.h: the cosine-weighted mean of the rows of --coldstart_donors content "
               "neighbours, no sampled article a donor) — and prints their Recall@20 and MRR@20 side by side: what a warm-started "
               "row is worth.  The engine is left byte for byte as found.  Needs --eval_panel; not with --dp_mode sharded or "
               "--gpus > 1.  0: off",
               (Rule("type", (int, float, np.integer, np.floating), "--eval_coldstart must be a number (0: off)"),
                Rule("finite", None, "--eval_coldstart must be a fraction in (0, 0.5] (0: off)"),
                Rule("range", (None, 0.5, None), "--eval_coldstart must be at most 0.5: the donors are the articles that are NOT sampled"),
                Rule("engine", "one", "--eval_coldstart rewrites item rows of ONE engine with the whole catalog; it cannot be combined with "
                                      "--dp_mode sharded"),
                Rule("one_process", None, "--eval_coldstart cannot be combined with --gpus > 1: the ranks would have to agree on the rows"),
                Rule("needs", "eval_panel", "--eval_coldstart needs --eval_panel P: its sessions are evaluated by the streamed evaluation"))),
    EvalOption("coldstart_donors", int,
               "K: the donors of one warm-started row under --eval_coldstart, 1 <= K <= %d (default %d)" % (MAX_DONORS, DEFAULT_DONORS),
               (Rule("type", (int, np.integer), "--coldstart_donors must be an integer in [1, %d]" % MAX_DONORS),
                Rule("range", (1, MAX_DONORS, None), "--coldstart_donors must be in [1, %d]" % MAX_DONORS))),
)
COLD_START_FLAGS = ("eval_coldstart", "coldstart_donors")


class ColdStartRequest(NamedTuple):
    frac: float
    donors: int


def check_cold_start_options(values, gpus=1):
    """refuse an --eval_coldstart / --coldstart_donors that cannot work: `values` as cli.check_eval_options takes them (dp_mode,
    eval_panel and the names of COLD_START_OPTIONS), the first broken rule as a ValueError"""
    cli.check_eval_options(values, gpus=gpus, options=COLD_START_OPTIONS)


def cold_start_request(model, args, req) -> Optional[ColdStartRequest]:
    """the cold-start pass of a test() call: `args` over the values the model was built with, else off; refused as the command
    line refuses it -> None where it is off"""
    values = {o.name: args.get(o.name, getattr(model, o.name, 0)) or 0 for o in COLD_START_OPTIONS}
    if not any(values.values()):
        return None
    gpus = max(int(args.get('gpus', 1) or 1), getattr(model, 'dp_world', 1))
    check_cold_start_options(dict(values, dp_mode=args.get('dp_mode', 'replica'), eval_panel=req.eval_panel), gpus=gpus)
    if not values["coldstart"]:
        return None
    return ColdStartRequest(float(values["coldstart"]), int(values["coldstart_donors"]) or DEFAULT_DONORS)


def cold_sample(labels, frac: float, seed: int) -> np.ndarray:
    """the articles --eval_coldstart treats as cold: round(frac * A) of the A distinct label articles (at least one), drawn
    without replacement by a RandomState(seed) of its own -> sorted int64 ids.  A function of the labels' SET, frac and seed."""
    arts = np.unique(np.asarray(labels, dtype=np.int64))
    if not arts.size:
        return arts
    take = min(arts.size, max(1, int(round(frac * arts.size))))
    return np.sort(np.random.RandomState(seed).choice(arts, size=take, replace=False))


def _take(feed, mask):
    """the sessions of a rectangular feed that `mask` names: every per-session entry restricted, everything else as it is"""
    B = len(mask)
    out = {}
    for name, v in feed.items():
        if isinstance(v, np.ndarray) and v.shape[:1] == (B,):
            out[name] = v[mask]
        elif isinstance(v, (list, tuple)) and len(v) == B:
            out[name] = [x for x, m in zip(v, mask) if m]
        else:
            out[name] = v
    return out


class ColdStart(EvalPass):
    """eval_coldstart FRAC (include/tcar_warm.h): what is a warm-started item row worth?  The pass needs every label of the data
    before it can draw its sample, so its engine calls are in `report`, behind the loop: it keeps the window of every streamed
    call (the feeds are the loop's own results), then evaluates the sessions whose label is sampled again with the sampled rows zeroed and with
    them warm-started.  The trained figures are the normal pass's own ranks, restricted.  It is the one pass that WRITES the engine:
    the rows go in through paths that leave the Adam moments alone (engine._hide_item_rows, _warm_start(zero_moments=False)), the
    old rows are kept on the device, and the restore puts back every byte — E, the planes, nothing else was touched."""
    key = "coldstart"

    def __init__(self, model, req, cold: ColdStartRequest):
        super().__init__(model, req)
        self.cold = cold

    def after_feed(self, feeds, bt, topk, window, rows_cap):
        self.kept.append((len(feeds), window))                      # (the feeds themselves are in the loop's results)

    def _evaluate(self, sample, results):
        """the streamed evaluation of the sessions whose label is in `sample`, one call per streamed call of the loop (its feeds
        are the next ones of `results`) -> their ranks, in the order of the loop"""
        ranks, at = [], 0
        for count, window in self.kept:
            feeds, at = [r.feed for r in results[at:at + count]], at + count
            masks = [np.isin(np.asarray(f["label"], dtype=np.int64).reshape(-1), sample) for f in feeds]
            subs = [_take(f, m) for f, m in zip(feeds, masks) if m.any()]
            if not subs:
                continue
            if window is not None:
                every = np.concatenate(masks)
                window = tuple(np.asarray(w)[every] for w in window)
            bt = self.eng.upload(subs[0] if len(subs) == 1 else pack_sessions(subs))
            rank, _, _ = self.eng.eval_step_streamed(None, k=20, bt=bt, panel=self.req.eval_panel, window=window,
                                                     max_per_category=self.req.cat_cap or None)
            ranks.append(rank.clone())
        return ranks

    def report(self, n, results):
        eng, k = self.eng, self.cold.donors
        labels = _labels([r.feed for r in results]) if results else np.zeros(0, np.int64)
        sample = cold_sample(labels, self.cold.frac, self.m.seed)
        ranks = {"trained": np.concatenate([r.rank.cpu().numpy() for r in results])[np.isin(labels, sample)] if results else np.zeros(0)}
        if sample.size:
            token = eng._hide_item_rows(sample)                     # the sampled rows := 0, the old rows stay on the device
            zeroed = self._evaluate(sample, results)
            eng._warm_start(*eng._warm_request(sample, k, 0.0, None, None, self.req.eval_panel), zero_moments=False)
            warm = self._evaluate(sample, results)
            eng._restore_item_rows(token)
            eng.check_forks()         # (synchronises) the figures below come from work enqueued behind test()'s own check
            for name, kept in (("zeroed", zeroed), ("warm", warm)):
                ranks[name] = np.concatenate([r.cpu().numpy() for r in kept]) if kept else np.zeros(0, np.int64)
        recall, mrr = {}, {}
        for name in ("trained", "zeroed", "warm"):
            h, m, _ = M.metrics_from_ranks(ranks.get(name, np.zeros(0)), 20)
            recall[name], mrr[name] = (float(np.mean(x)) if len(x) else 0.0 for x in (h, m))
        print('cold start ({} articles, {} donors): Recall@20 trained {}, zeroed {}, warm-started {}; MRR@20 {}, {}, {}'.format(
            int(sample.size), k, recall["trained"], recall["zeroed"], recall["warm"], mrr["trained"], mrr["zeroed"], mrr["warm"]))
        return {"articles": int(sample.size), "donors": k, "sessions": int(len(ranks["trained"])), "sample": sample.tolist(),
                "recall": recall, "mrr": mrr}


def active_passes(model, req, cold: Optional[ColdStartRequest] = None):
    """the passes that `req` turns on, in the order of the module's docstring; `cold`: the cold-start pass, behind all of them"""
    two = TwoStage(model, req) if req.eval_shortlist or req.shard_eval_shortlist else None
    return [p for p in (Candidates(model, req) if req.eval_candidates else None,
                        two,
                        Diversified(model, req, two) if req.eval_diversity and not req.shard_eval_shortlist else None,
                        Sections(model, req) if req.eval_sections else None,
                        Related(model, req) if req.eval_related else None,
                        LabelsOutside(model, req) if req.fresh_hours else None,
                        Capped(model, req) if req.cat_cap else None,
                        ColdStart(model, req, cold) if cold else None) if p is not None]
