"""`Seq2SeqAttNN` — host-side mirror of the reference's model plug-in (model_combine.py:10-315).

main.py:65-66 loads the model as ``getattr(__import__(args.model), "Seq2SeqAttNN")(args_dict)`` and calls
``train(sess, item_dict, train_data, neighbor_dict, args, test_data, saver)`` / ``test(sess, test_data, args)``.
This class keeps those signatures (``sess`` / ``saver`` are accepted and ignored: there is no TensorFlow session),
the stdout lines of model_combine.py:201,229-230,244,247,255,288-293,310-314 and the NaN guard (:243-246), and
runs every step on the HIP engine (`tcar_amd.engine.TcarEngine`).  Differences that are deliberate:

  * the per-batch feed is int32 arrays from the tensorised sampler (host/sampler.py), not nested lists;
  * evaluation ranks / top-20 come from the `tcar_rank_topk` kernel, so the [B, N] score matrix never travels to
    the host (model_combine.py:293,296,301 argsort it twice per session on the CPU);
  * ILD / unexp are vectorised over an int category table (model_combine.py:174-194 are O(20^2) dict lookups);
  * dense weights are drawn from RandomState(2020) (TF's RNG stream of tf.set_random_seed(2020) cannot be
    reproduced); the embedding tables consume the GLOBAL numpy stream in creation order exactly like
    modules.py:32, so a seeded run draws the same negatives as the reference afterwards.
"""
from __future__ import annotations

import os
import time
from collections import OrderedDict

import numpy as np
import torch

from ..engine import TIME_NAMES, TIME_VOCAB, TcarEngine, VAR_ORDER
from . import cli, metrics as M
from .data import pack_sessions, publish_fields
from .eval_passes import COLD_START_OPTIONS, FeedResult, active_passes, cold_start_request
from .sampler import Sampler


def _shapes(N, H, Ht):
    s = OrderedDict()
    s["item_emb"] = (N + 1, H)
    s["dec_pos"] = (40, H)
    for n, v in zip(TIME_NAMES, TIME_VOCAB):
        s[n] = (v, Ht)
    s["duration_embedding"] = (11, Ht)
    dense = {"multi_attention/input_linear_trans/w_3d": (2 * H, H), "multi_attention/cont_linear_trans/w_3d": (H, H),
             "multi_attention/inter_linear_trans/w_3d": (Ht, H), "multi_attention/res_linear_trans/w_3d": (H, 1),
             "multi_attention/query_trans1/w1": (2 * Ht, H), "multi_attention/query_trans1/b1": (H,),
             "multi_attention/query_trans2/w1": (H, 2 * H), "multi_attention/query_trans2/b1": (2 * H,),
             "attout_item_cont_trans/w1": (2 * H, 2 * H), "attout_item_cont_trans/b1": (2 * H,),
             "cont_attention/input_linear_trans/w_3d": (5 * Ht, H), "cont_attention/cont_linear_trans/w_3d": (H, H),
             "cont_attention/res_linear_trans/w_3d": (H, 1), "attout_pt_trans/w1": (5 * Ht, 5 * Ht),
             "attout_pt_trans/b1": (5 * Ht,)}
    for n in VAR_ORDER:
        if n in dense:
            s[n] = dense[n]
    return s


def initial_variables(N, H, Ht, emb_stddev, stddev, weight_seed=2020, lean=False):
    """Tables: np.random.normal on the global stream, creation order, row 0 zeroed when zero_pad
    (modules.py:32-34; dec_pos default stddev 0.02 and no pad, model_combine.py:57-64; duration no pad, :106).
    Dense weights ~ N(0, stddev) (modules.py:50-51,65) from a private stream.
    lean=True (multi-million-item catalogs): the item table is drawn in fp32 row chunks from a private generator (the
    fp64 draw of a 10M x 256 table alone is 20 GB)."""
    wr = np.random.RandomState(weight_seed)
    out = OrderedDict()
    for name, shp in _shapes(N, H, Ht).items():
        if name == "item_emb" and lean:
            g32 = np.random.default_rng(weight_seed + 1)
            t = np.empty(shp, dtype=np.float32)
            for lo in range(0, shp[0], 1 << 20):
                hi = min(shp[0], lo + (1 << 20))
                t[lo:hi] = g32.standard_normal((hi - lo, shp[1]), dtype=np.float32) * np.float32(emb_stddev)
            t[0] = 0.0
            out[name] = t
            continue
        if name == "dec_pos":
            t = np.random.normal(0, 0.02, shp)
        elif name in ("item_emb", "duration_embedding") or name in TIME_NAMES:
            t = np.random.normal(0, emb_stddev, shp)
            if name != "duration_embedding":
                t[0] = 0.0
        else:
            t = wr.normal(0, stddev, shp)
        out[name] = t.astype(np.float32)
    return out


def _idx0(sampler, i: int) -> int:
    """store row of the first example of batch i (its input length is the batch's T)"""
    return int(sampler.batch_indices(i)[0])


def prefetch_batches(sampler, depth: int = 4):
    """Iterate sampler.next_batch_arrays() from a producer thread (same order, same RNG stream: only this thread draws
    from numpy's global generator while it runs) so batch assembly overlaps the upload / step enqueue of the consumer;
    the ctypes step call and the H2D copy release the GIL."""
    import queue
    import threading
    q = queue.Queue(maxsize=depth)
    END = object()

    def produce():
        try:
            while sampler.has_next():
                q.put(sampler.next_batch_arrays())
            q.put(END)
        except BaseException as e:          # surfaced in the consumer
            q.put(e)

    th = threading.Thread(target=produce, daemon=True)
    th.start()
    while True:
        item = q.get()
        if item is END:
            break
        if isinstance(item, BaseException):
            raise item
        yield item
    th.join()


class Seq2SeqAttNN():
    """The memory network with context/temporal attention, MI355X edition."""

    def __init__(self, args):
        self.publish_time_MWDHM = np.array(args['publish_time_MWDHM'], dtype=np.int32)      # (a copy: update_articles writes it)
        self.itemnum = args['itemnum']
        self.category_id = args['category_id']
        self.item_freq_dict_norm = args.get('item_freq_dict_norm')
        self.reverse_item = args['reverse_item']
        content = np.asarray(args['content_emb'], dtype=np.float32)
        self.candidate_n = content.shape[0]
        self.emb_stddev = args['emb_stddev']
        self.stddev = args['stddev']
        self.hidden_size = args['hidden_size']
        self.time_hidden_size = args['time_hidden_size']
        self.l2_emb = args.get('l2_emb', 0.0)
        self.batch_size = args['batch_size']
        self.epoch = args['epoch']
        self.neg_num = args['neg_num']
        self.gap_mode = args.get('gap_mode', 'active_t')
        self.neg_mode = args.get('neg_mode', 'uniform')
        self.neg_fast = bool(args.get('neg_fast', 0))
        self.device_sampler = bool(args.get('device_sampler', 0))   # form batches + draw negatives on the GPU
        self.seed = int(args.get('seed', 2020))
        # test(): the evaluation options this model is built with (cli.EVAL_OPTIONS: eval_panel ... eval_mixed), each under its name
        for name, value in self._eval_request(args)._asdict().items():
            setattr(self, name, value)
        for opt in COLD_START_OPTIONS:                               # (eval_passes.cold_start_request checks them, in test())
            setattr(self, opt.name, args.get(opt.name, 0) or 0)
        self.publish_time = args.get('publish_time')                # per-item datetimes (the keys of a window), as the fold loader returns them
        self._keys = self._key_t0 = None
        self._ds_cache = {}
        self.curEpoch = 0
        self.error_during_train = False
        if content.shape[1] != self.hidden_size:
            raise ValueError("content_emb width %d != --hidden_size %d (model_combine.py:111 concatenates them)"
                             % (content.shape[1], self.hidden_size))
        N = self.candidate_n - 1
        print('size of seq_content', (None, None, self.hidden_size))
        print('size of seq_publish_t', (None, None, 5 * self.time_hidden_size))
        print('size of click_t', (None, 2 * self.time_hidden_size))
        params = args.get('initial_variables') or initial_variables(N, self.hidden_size, self.time_hidden_size,
                                                                    self.emb_stddev, self.stddev)
        self.variables_names = [n + ':0' for n in VAR_ORDER]
        print(self.variables_names)
        engine_cls = TcarEngine
        kw = {}
        if args.get('dp_group') is not None:
            from ..dp import DPEngine
            engine_cls, kw = DPEngine, {"group": args['dp_group']}
            if args.get('dp_mode', 'replica') == 'sharded':
                from ..sharded import ShardedEngine
                engine_cls = ShardedEngine
        elif self.shard_eval_panel:             # one process, no group: the catalog-sharded engine with ONE shard (no collective runs)
            from ..sharded import ShardedEngine
            engine_cls = ShardedEngine
        self.engine = engine_cls(params, content, self.publish_time_MWDHM, lr=args['lr'], max_grad=args.get('max_grad'),
                                 device=args.get('device', 'cuda:0'), scoring=args.get('scoring', 'bf16x3-mixed'), **kw)
        self._cat = None
        self._store_cache = {}
        # data parallel (main.py --gpus N): every rank builds the SAME batches (same seeds) and keeps its contiguous shard
        self.dp_group = args.get('dp_group')
        if self.dp_group is not None:
            import torch.distributed as dist
            self.dp_rank, self.dp_world = dist.get_rank(self.dp_group), dist.get_world_size(self.dp_group)
        else:
            self.dp_rank, self.dp_world = 0, 1

    def _eval_request(self, args) -> cli.EvalRequest:
        """the evaluation options of a test() call: for every option `args` over the value the model was built with, else off,
        refused as the command line refuses them (cli.check_eval_options: the first broken rule, in its order)"""
        values = {}
        for opt in cli.EVAL_OPTIONS:
            v = args.get(opt.name, getattr(self, opt.name, 0)) or 0
            # (an option with a rule about its type is checked as it came, the others as the number they stand for)
            values[opt.name] = v if opt.rules[0].kind == "type" else opt.type(v)
        gpus = max(int(args.get('gpus', 1) or 1), getattr(self, 'dp_world', 1))
        cli.check_eval_options(dict(values, dp_mode=args.get('dp_mode', 'replica')), gpus=gpus)
        return cli.EvalRequest(**{opt.name: opt.type(values[opt.name]) for opt in cli.EVAL_OPTIONS})

    def _packs(self, feeds, mixed: bool):
        """test(): the sampler's feeds grouped into the packs of one streamed call each — consecutive feeds, never splitting one,
        while the pack holds at most batch_size sessions (eval_mixed); without the flag every feed is its own pack"""
        pack, n = [], 0
        for feed in feeds:
            b = int(feed["seq"].shape[0])
            if pack and (not mixed or n + b > self.batch_size):
                yield pack
                pack, n = [], 0
            pack.append(feed)
            n += b
        if pack:
            yield pack

    def _label_among_sampled(self, labels, ncand: int, rng):
        """candidate lists [B, ncand] of the "label among sampled negatives" protocol: the label in slot 0, then ncand - 1 items drawn
        uniformly from the catalog without the label (repeats among them allowed), and the matching clicked flags"""
        lab = np.asarray(labels, dtype=np.int64).reshape(-1, 1)
        others = rng.randint(0, self.candidate_n - 2, size=(lab.shape[0], ncand - 1)).astype(np.int64)
        others += others >= lab                      # uniform over the N - 1 items that are not the label
        clicked = np.zeros((lab.shape[0], ncand), dtype=np.int32)
        clicked[:, 0] = 1
        return np.concatenate([lab, others], axis=1).astype(np.int32), clicked

    # ------------------------------------------------------------------------------------------ helpers
    def _category_table(self):
        if self._cat is None:
            self._cat = M.category_table(self.reverse_item, self.category_id, self.candidate_n - 1)
        return self._cat

    def printData(self, filename, batch_in, batch_out, batch_pred):
        os.makedirs('saved', exist_ok=True)
        with open('saved/CAR+P_Normal_predict_exa_' + filename + '.txt', 'a+') as f:
            for index in range(len(batch_in)):
                f.write('# batch in: {} # batch out: {} # batch pred: {} \n'.format(
                    str(batch_in[index]), str(batch_out[index]), str(batch_pred[index])))

    def getILD(self, recList):
        return float(M.ild_batch(np.asarray([recList]), self._category_table())[0])

    def getUnexp(self, inSeq, recList):
        if len(recList) == 0:
            return 0
        return float(M.unexp_batch(np.asarray([inSeq]), np.asarray([recList]), self._category_table())[0])

    def _install_categories(self):
        """the category table on the engine (set_categories), once per table: what eval_diversity and max_per_category read"""
        cat = self._category_table()
        if getattr(self, "_cat_on_engine", None) is not cat:
            self.engine.set_categories(cat)
            self._cat_on_engine = cat

    def _item_keys(self):
        """int32 key of every item = its publish time in minutes since the earliest one; installed on the engine once"""
        if self._keys is None:
            pt = self.publish_time
            if pt is None or len(pt) != self.candidate_n - 1 or any(t is None for t in pt):
                raise ValueError("a publish-time window needs args['publish_time']: one datetime per item, none of them None")
            ts = np.asarray(pt, dtype="datetime64[s]")
            self._key_t0 = ts.min()
            minutes = (ts - self._key_t0).astype(np.int64) // 60
            if int(minutes.max()) >= 2 ** 31 - 1:
                raise ValueError("publish times span more minutes than an int32 key holds")
            self._keys = minutes.astype(np.int32)
            self.engine.set_item_keys(self._keys)
        return self._keys

    def minute_of(self, when) -> np.ndarray:
        """datetimes -> the minutes of the item keys (since the earliest publish time): the unit of a window's bounds"""
        self._item_keys()
        return (np.asarray(when, dtype="datetime64[s]") - self._key_t0).astype(np.int64) // 60

    def _fresh_window(self, feed, time_dict, hours):
        """the pools of a test batch: hi = the minute of the label's click + 1, lo = hi - 60 hours -> (lo, hi)"""
        T = feed["seq"].shape[1]
        hi = self.minute_of([time_dict[key][T]['click_t'] for key in feed["keys"]]) + 1
        return hi - int(round(60 * hours)), hi

    def _sampler(self, data, neighbor_dict=None, item_dict=None, neg_num=None):
        # (len_dict, session_dict, session_time_dict) as util.py:56 returns it, or with a 4th element: a prebuilt
        # SessionStore whose integer example ids populate len_dict (large synthetic folds skip the dict form)
        len_d, sess_d, time_d = data[:3]
        store = data[3] if len(data) > 3 else None
        return Sampler(len_d, sess_d, time_d, neighbor_dict, item_dict, neg_num, batch_size=self.batch_size,
                       gap_mode=self.gap_mode, neg_mode=self.neg_mode, store=store, neg_fast=self.neg_fast)

    def _device_batches(self, data, sampler, neighbor_dict, item_dict, K):
        """Iterate C batch descriptors formed ON THE DEVICE (device_sampler.DeviceSampler): the host sampler has only done
        the bucketed shuffle (sampler.py:40-49); each batch costs one H2D copy of its example indices."""
        from ..device_sampler import DeviceSampler
        store = sampler.store
        mode = self.neg_mode if (neighbor_dict and K) else "uniform"
        key = (id(store), mode)
        ds = self._ds_cache.get(key)
        if ds is None:
            ds = self._ds_cache[key] = DeviceSampler(self.engine, store, mode, neighbor_dict if mode != "uniform" else None,
                                                     item_dict, seed=self.seed)
        k = K if (neighbor_dict and K) else 0
        if self.dp_world == 1:
            # the epoch's example indices go up ONCE; every feed is then formed from HBM-resident data, one batch ahead of the
            # step on a side stream (DeviceSampler.planned) — nothing crosses PCIe inside the epoch
            ds.plan([sampler.batch_indices(i) for i in range(sampler.batch_num)])
            for bt in ds.planned(k, self.gap_mode):
                yield bt, None, None
            return
        for i in range(sampler.batch_num):
            idx = sampler.batch_indices(i)
            if self.dp_world > 1:
                from ..dp import shard_bounds
                lo, hi, cap = shard_bounds(len(idx), self.dp_world, self.dp_rank)
                T = int(store.in_len[idx[0]])
                yield (ds.form(idx[lo:hi], k, self.gap_mode) if hi > lo else None), cap * T, idx[lo:hi]
            else:
                yield ds.form(idx, k, self.gap_mode), None, idx

    def _shard(self, feed):
        """this rank's contiguous shard of a batch (dp.shard_bounds) -> (sub-feed or None when empty, rows capacity / T)"""
        if self.dp_world == 1:
            return feed, None
        from ..dp import shard_bounds
        b = feed["seq"].shape[0]
        lo, hi, cap = shard_bounds(b, self.dp_world, self.dp_rank)
        if hi <= lo:
            return None, cap
        return {k: (v[lo:hi] if v is not None else None) for k, v in feed.items()}, cap

    def _allsum(self, values):
        """sum a list of python floats over the ranks"""
        if self.dp_world == 1:
            return values
        import torch.distributed as dist
        t = torch.tensor(values, dtype=torch.float64, device=self.engine.dev)
        dist.all_reduce(t, group=self.dp_group)
        return t.cpu().tolist()

    # -------------------------------------------------------------------------------------------- train
    def train(self, sess, item_dict, train_data, neighbor_dict, args, test_data=None, saver=None, threshold_acc=0.99):
        eng = self.engine
        for epoch in range(self.epoch):
            self.curEpoch = epoch
            print('Epoch {}'.format(epoch))
            batch = 0
            sampler = self._sampler(train_data, neighbor_dict, item_dict, args['neg_num'])
            # per-row fp64 accumulator of the epoch's losses: ONE small kernel per step (the reference sums python floats)
            acc = torch.zeros(max(int(args['batch_size']), 1), dtype=torch.float64, device=eng.dev)
            count = 0
            t0 = time.time()
            if self.device_sampler:
                for bt, cap_rows, _idx in self._device_batches(train_data, sampler, neighbor_dict, item_dict, args['neg_num']):
                    batch += 1
                    if self.dp_world > 1:
                        crt_loss = eng.train_step(None, bt=bt, cap_rows=cap_rows, T=int(sampler.store.in_len[_idx0(sampler, batch - 1)]),
                                                  K=args['neg_num'] if neighbor_dict else 0)
                    else:
                        crt_loss = eng.train_step(None, bt=bt, defer_update=True)   # applied inside the next step (flush below)
                    acc[:crt_loss.numel()].add_(crt_loss)
                    count += crt_loss.numel()
            for feed in (() if self.device_sampler else prefetch_batches(sampler)):
                batch += 1
                if batch < 3 and feed["neg"] is not None:
                    print(feed["neg"][0][:10].tolist())
                if self.dp_world > 1:
                    T = feed["seq"].shape[1]
                    sub, cap = self._shard(feed)
                    crt_loss = eng.train_step(sub, cap_rows=cap * T, T=T, K=(feed["neg"].shape[1] if feed["neg"] is not None else 0))
                else:
                    crt_loss = eng.train_step(feed, defer_update=True)   # [b] on device; no host sync inside the loop
                acc[:crt_loss.numel()].add_(crt_loss)
                count += crt_loss.numel()
            eng.flush()                                         # the last step's deferred update
            eng.check_forks()
            tot, cnt = self._allsum([float(acc.sum().item()), float(count)])
            avgc = tot / max(cnt, 1)
            self.train_seconds = time.time() - t0
            self.train_sessions = int(cnt)
            if np.isnan(avgc):
                print('Epoch {}: NaN error!'.format(str(epoch)))
                self.error_during_train = True
                return
            print('\tloss: {:.6f}'.format(avgc))
            if test_data is not None:
                recall = self.test(sess, test_data, args)
                if recall > threshold_acc:       # every rank takes part (the sharded export is a collective), rank 0 writes
                    modelname = self.save(args)
                    if self.dp_rank == 0:
                        print('Model saved - {}'.format(modelname))

    def save(self, args):
        suf = time.strftime("%Y%m%d%H%M", time.localtime()) + '-' + str(args.get('dataset', '')).replace('/', '_') \
            + '-' + str(args.get('split_way', '')).replace('/', '_') + '-' + str(args.get('foldnum', 0))
        path = os.path.join(args.get('modelpath', './ckpt/'), "model.ckpt-" + suf + ".npz")
        # plain arrays only (variables, Adam moments, beta powers, step): loadable without unpickling anything.  NOT
        # interchangeable with the reference's tf.train.Saver checkpoints (README.md).
        state = self.engine.export_state()          # catalog-sharded engine: all-gathers the owners' Adam moments
        if self.dp_rank == 0:                       # replicas are identical: one writer
            os.makedirs(os.path.dirname(path) or '.', exist_ok=True)
            np.savez(path, **state)
        return path

    # --------------------------------------------------------------------------------------------- test
    @staticmethod
    def _print_batch(feed, tk, args):
        """the lines test() prints for its first two feeds (tk: the top-k list of the feed's first session)"""
        print('batch_in:', feed["seq"][0].tolist())
        print('active_interval:', feed["gap"][0].tolist())
        print('input_click_week:', int(feed["cw"][0]))
        print('batch_out:', int(feed["label"][0]), args['publish_time'][int(feed["label"][0])])
        print('batch pred:', tk[:10])

    def test(self, sess, test_data, args):
        """The evaluation loop.  Per streamed call its engine calls come in ONE order: the streamed (or materialised) evaluation,
        eval_diversity for every feed of the call, then the optional passes in the order of eval_passes.active_passes.  Everything
        kept of a feed is a clone on the device: but for the lists printed of the first two feeds, nothing is copied to the host and
        nothing synchronises before check_forks()."""
        print('Measuring...')
        eng = self.engine
        req = self._eval_request(args)
        if req.eval_candidates and self.candidate_n - 1 < 2:
            raise ValueError("eval_candidates ranks the label among OTHER items: the catalog holds fewer than two")
        if req.shard_eval_panel and not hasattr(eng, "xch"):
            raise ValueError("shard_eval_panel needs the catalog-sharded engine (dp_mode sharded when the model is built)")
        time_dict = test_data[2] if len(test_data) > 2 else None
        if req.fresh_hours:
            if not time_dict:
                raise ValueError("fresh_hours takes the label's click time from the fold's session_time_dict, which this fold lacks")
            self._item_keys()
        sampler = self._sampler(test_data)
        # ILD / unexp pair counts and the set of recommended items stay on the device (tcar_eval_diversity)
        self._install_categories()
        eng.reset_coverage()
        passes = active_passes(self, req, cold_start_request(self, args, req))
        panel, mixed = req.eval_panel or req.shard_eval_panel, bool(req.eval_mixed)
        keep_lists = args.get('is_print') or req.cat_cap
        results, batch, eval_calls = [], 0, 0
        # One streamed call per pack of feeds.  eval_mixed packs feeds of different lengths into a ragged batch (include/tcar_ragged.h;
        # a pack of one feed goes the rectangular way); without it every feed is its own pack.  The sessions of a feed are contiguous
        # in the pack and their flat rows are its [B_g, T_g] block, so the diversity counts are taken per feed on that block of the
        # uploaded batch and on the feed's rows of topk.
        for pack in self._packs(prefetch_batches(sampler), mixed):
            eval_calls += 1          # (data parallel: a collective step, the same count on every rank)
            rows_cap = None
            if not mixed:            # data parallel: every rank scores its shard of the batch
                T = pack[0]["seq"].shape[1]
                feed, rows_cap = self._shard(pack[0])
                if feed is None:     # the sharded calls are COLLECTIVES: a rank without sessions still joins every exchange
                    batch += 1
                    if req.shard_eval_panel:
                        eng.eval_step_streamed(None, k=20, panel=panel, cap=rows_cap, T=T)
                    for p in passes:
                        p.idle(rows_cap, T)
                    continue
                pack = [feed]
            bt = eng.upload(pack_sessions(pack) if len(pack) > 1 else pack[0])
            window = None
            if req.fresh_hours:
                window = tuple(np.concatenate(w) for w in zip(*[self._fresh_window(f, time_dict, req.fresh_hours) for f in pack]))
            if panel:                # streamed: no [B, N] score matrix; inside the sessions' pools (fresh_hours), capped per category
                rank, topk, ce = eng.eval_step_streamed(None, k=20, bt=bt, panel=panel, window=window, max_per_category=req.cat_cap or None,
                                                        **({"cap": rows_cap} if req.shard_eval_panel else {}))
            else:
                rank, topk, ce = eng.eval_step(None, k=20, bt=bt)
            s0 = r0 = 0
            for feed in pack:
                batch += 1
                b, T = feed["seq"].shape
                rows, block = (slice(s0, s0 + b), (r0, b, T)) if mixed else (slice(None), None)
                tk = topk[rows]
                ild_c, unexp_c, n_rec = eng.eval_diversity(bt, tk, block=block)
                results.append(FeedResult(feed, rank[rows].clone(), tk.clone() if keep_lists else None, ce[rows].clone(), ild_c, unexp_c, n_rec))
                if batch < 3:
                    self._print_batch(feed, tk[0].cpu().numpy().tolist(), args)
                s0, r0 = s0 + b, r0 + b * T
            for p in passes:
                p.after_feed(pack, bt, topk, window, rows_cap)
        eng.check_forks()             # (synchronises) nothing below is reported from a run whose flag forks timed out
        hits, mrrs, ndcgs, ilds, unexps, losses = [], [], [], [], [], []
        for r in results:
            h, m, n = M.metrics_from_ranks(r.rank.cpu().numpy(), 20)
            hits += h.tolist()
            mrrs += m.tolist()
            ndcgs += n.tolist()
            losses += r.ce.cpu().numpy().tolist()
            il, un = M.diversity_from_counts(r.ild_c.cpu().numpy(), r.unexp_c.cpu().numpy(), r.n_rec.cpu().numpy(), r.feed["seq"].shape[1])
            ilds += il.tolist()
            unexps += un.tolist()
            if args.get('is_print'):
                self.printData(str(args['foldnum']) + '_' + str(self.curEpoch), r.feed["seq"].tolist(),
                               r.feed["label"].tolist(), r.topk.cpu().numpy().astype(np.int64).tolist())
        # sums over this rank's sessions, then over the ranks; coverage = union of the recommended items
        sums = self._allsum([float(np.sum(x)) for x in (losses, ilds, unexps, mrrs, hits, ndcgs)] + [float(len(hits))])
        n = max(sums[6], 1.0)
        if self.dp_world > 1:
            import torch.distributed as dist
            dist.all_reduce(eng._seen, op=dist.ReduceOp.MAX, group=self.dp_group)      # union of the ranks' byte maps
        n_covered = eng.coverage()
        m_loss, m_ild, m_unexp, m_mrr, m_hit, m_ndcg = [v / n for v in sums[:6]]
        print('avg loss...', m_loss)
        print('avg ILD...', m_ild)
        print('avg unexp...', m_unexp)
        print('len of result dict: ', n_covered)
        print('MRR@20: {}, Recall@20: {}, nDCG@20: {}'.format(m_mrr, m_hit, m_ndcg))
        self.last_metrics = {"mrr": m_mrr, "recall": m_hit, "ndcg": m_ndcg, "loss": m_loss, "ild": m_ild,
                             "unexp": m_unexp, "coverage": n_covered, "eval_calls": eval_calls, "sessions": int(sums[6])}
        for p in passes:              # every rank, every pass, this order: their sums over the ranks are collectives
            self.last_metrics[p.key] = p.report(n, results)
        return m_hit

    # ---------------------------------------------------------------------------------------- recommend
    def recommend(self, sessions, k=20, window=None, max_per_category=None, shortlist=None, diversity=None, **kw):
        """The k best next items of every session of `sessions` — a feed dict as the samplers build it (seq, pm, pd, pw, ph, pmi,
        gap, cw, ch; no label, no neg) — as (topk [B, k] int32 0-based ids, scores [B, k] f32) on the device; items the session
        has already read are left out (engine.TcarEngine.recommend has the options).  window = (lo, hi), scalars or arrays [B], in
        minutes since the earliest publish time (`minute_of(datetime)`): only items published in [lo, hi) are candidates.
        max_per_category = m >= 1: at most m items of one category (the fold's category table) in a list.
        With the catalog-sharded engine (dp_mode sharded) this is a COLLECTIVE: every rank calls it with its own sessions — None
        where it has none, with cap= and T= (sharded.ShardedEngine.recommend).
        shortlist = C (k <= C <= 1024): the two-stage form — C items retrieved from coarse scores, re-scored exactly, the k best of
        them returned (engine.TcarEngine.recommend_two_stage; the catalog-sharded engine: shard_recommend_two_stage, a collective
        like its recommend); None: the streamed selection over exact scores, as ever.
        diversity = mu >= 0 (only with shortlist): the k items are taken from the shortlist by the MMR walk over content
        (engine.TcarEngine.recommend_two_stage: a verbatim duplicate of a listed item loses mu logits); refused by the
        catalog-sharded engine."""
        if diversity is not None and shortlist is None:
            raise ValueError("diversity re-ranks the shortlist of the two-stage recommendation: pass shortlist=C with it")
        if shortlist is not None and max_per_category is not None:
            raise ValueError("the two-stage recommendation takes no per-category cap (shortlist and max_per_category exclude each other)")
        sessions = self._feed(sessions)
        if window is not None:
            self._item_keys()
        if max_per_category is not None:
            self._install_categories()
        if shortlist is not None:
            two_stage = self.engine.shard_recommend_two_stage if self._sharded() else self.engine.recommend_two_stage
            if diversity is not None:
                kw = dict(kw, diversity=diversity)
            return two_stage(sessions, k=k, shortlist=shortlist, window=window, **kw)
        return self.engine.recommend(sessions, k=k, window=window, max_per_category=max_per_category, **kw)

    def recommend_sections(self, sessions, sections, k=10, window=None, **kw):
        """One list per CATEGORY for every session of `sessions` — a feed dict as `recommend` takes it: `sections` names G codes of
        the fold's category table (1 <= G <= 16, pairwise distinct), and list g holds the k best items of category sections[g].
        engine.SectionLists(topk [B, G, k] int32 0-based ids, scores [B, G, k] f32, overall_topk, overall_scores) on the device, from
        ONE pass over the catalog (engine.TcarEngine.recommend_sections has the options: exclude_seen, exclude, panel, overall).
        window as in `recommend`: "fresh sport" is a section inside a publish-time window.  Not on the catalog-sharded engine."""
        sessions = self._feed(sessions)
        self._install_categories()
        if window is not None:
            self._item_keys()
        return self.engine.recommend_sections(sessions, sections, k=k, window=window, **kw)

    def related_articles(self, ids, k=10, window=None, max_per_category=None, **kw):
        """The k articles whose CONTENT is most similar to each article of `ids` (int [Q], 0-based as the lists `recommend` returns):
        (topk [Q, k] int32, cosines [Q, k] f32) on the device, best first, the article itself left out, -1 where fewer than k are
        eligible.  No session and no model: the cosine of the frozen content rows, the one the diversity re-rank charges
        (engine.TcarEngine.similar_items has the options: exclude_self, exclude, panel).  window = (lo, hi), scalars or arrays [Q],
        in minutes since the earliest publish time, and max_per_category as in `recommend`.  Not on the catalog-sharded engine."""
        return self._similar(dict(ids=ids), k, window, max_per_category, kw)

    def similar_to_content(self, rows, k=10, window=None, max_per_category=None, **kw):
        """`related_articles` for rows that are in no catalog — float [Q, H] content vectors, e.g. a draft before update_articles
        publishes it: is this story already in the catalog?"""
        return self._similar(dict(content=rows), k, window, max_per_category, kw)

    def _similar(self, query, k, window, max_per_category, kw):
        if window is not None:
            self._item_keys()
        if max_per_category is not None:
            self._install_categories()
        return self.engine.similar_items(k=k, window=window, max_per_category=max_per_category, **query, **kw)

    def duplicate_articles(self, threshold=0.98, window=None, **kw):
        """Which articles of the catalog are copies of each other: (groups, audit).  `audit` is what engine.TcarEngine.find_duplicates
        returns — for every article the number of others whose content cosine with it is >= threshold, the most similar of them and
        its cosine, on the device — and `groups` the best-partner clusters of host.metrics.duplicate_groups: sorted lists of 0-based
        ids, two or more each.  window = (lo, hi), ONE pair of scalars in minutes since the earliest publish time
        (`minute_of(datetime)`): only the articles published in [lo, hi) are audited, against each other — e.g. the fresh window
        behind update_articles.  Not on the catalog-sharded engine."""
        from .metrics import duplicate_groups
        if window is not None and not self._sharded():
            self._item_keys()
        audit = self.engine.find_duplicates(threshold=threshold, window=window, **kw)
        return duplicate_groups(audit.partner.cpu().numpy()), audit

    def retrieve(self, sessions, C, window=None, **kw):      # noqa: N803
        """A shortlist of the C best next items (1 <= C <= 1024) of every session of `sessions` — a feed dict as `recommend` takes
        it — from coarse scores: (ids [B, C] int32, coarse_scores [B, C] f32) on the device, -1 / -inf where fewer than C items are
        eligible; a valid `candidates` of score_candidates (engine.TcarEngine.retrieve has the options).  window as in `recommend`.
        With the catalog-sharded engine a COLLECTIVE, as `recommend` (sharded.ShardedEngine.shard_retrieve: cap= and T=)."""
        if window is not None:
            self._item_keys()
        call = self.engine.shard_retrieve if self._sharded() else self.engine.retrieve
        return call(self._feed(sessions), C, window=window, **kw)

    # ---------------------------------------------------------------------------------- catalog updates
    def update_articles(self, ids, content=None, publish_time=None, category=None, item_rows=None, donors=16, donor_window=None):
        """Publish, correct or retire articles in the live engine (engine.TcarEngine.update_items; one call of it): ids int [U] in
        the id convention of the lists `recommend` returns (0-based), then any of content float [U, H], publish_time (U datetimes),
        category int [U] (codes of the fold's category table) and item_rows float [U, H] (new item-table rows; their Adam moments
        start from zero).  From publish_time come the publish_time_MWDHM rows — the fold loader's fields, host.data.publish_fields —
        and, once the item keys are installed (a window has been used), the minute keys since the earliest publish time the keys
        were built from; a time before it is refused.  The model's own tables (publish_time_MWDHM, publish_time, the keys, the
        category table) follow the engine's.
        The neighbour-negative lists of the sampler are NOT rebuilt: training after an update draws negatives from the lists the
        fold was loaded with.
        Routed by engine, as score_candidates: the catalog-sharded engine takes it as shard_update_items, the data-parallel replicas
        as replica_update_items, any other engine as update_items.  On the first two EVERY rank calls update_articles with the same
        arguments — as every rank already builds the same batches — and the ranks check that they did (dp.Collectives.agree).
        item_rows="neighbors": the update of content, time, key and category runs first, then `warm_start_articles(ids, donors,
        donor_window)` gives the rows the cosine-weighted mean of the trained rows of their `donors` nearest content neighbours
        (engine.TcarEngine.warm_start_items) — what a new article gets instead of the spare row's noise.  One engine with the whole
        catalog only.  Any other string is a ValueError."""
        ids = np.asarray(ids)
        neighbors = isinstance(item_rows, str)
        if neighbors:
            if item_rows != "neighbors":
                raise ValueError('item_rows must be an array [U, H], None or the string "neighbors" (got %r)' % item_rows)
            self._refuse_warm_start()
            item_rows = None
            if content is None and publish_time is None and category is None:      # nothing but the warm start
                self.warm_start_articles(ids, donors=donors, window=donor_window)
                return
        mw = keys = None
        if publish_time is not None:
            when = list(publish_time)
            mw = np.asarray([publish_fields(t) for t in when], dtype=np.int32).reshape(len(when), 5)
            if self._keys is not None:
                keys = self.minute_of(when)
                if keys.size and int(keys.min()) < 0:
                    raise ValueError("publish_time before the earliest publish time of the item keys (%s): the keys count minutes since it"
                                     % self._key_t0)
        if category is not None:
            self._install_categories()
        call = (self.engine.shard_update_items if self._sharded() else
                self.engine.replica_update_items if hasattr(self.engine, "replica_update_items") else self.engine.update_items)
        call(ids, content=content, item_rows=item_rows, mwdhm=mw, keys=keys, categories=category)
        if publish_time is not None:
            self.publish_time_MWDHM[ids] = mw
            if self.publish_time is not None:
                if not isinstance(self.publish_time, (list, np.ndarray)):
                    self.publish_time = list(self.publish_time)
                for i, t in zip(ids.tolist(), when):
                    self.publish_time[i] = t
            if keys is not None:
                self._keys[ids] = keys.astype(np.int32)
        if category is not None:
            self._cat[ids] = np.asarray(category)          # in place: the table on the engine stays THIS table (_cat_on_engine)
        if neighbors:
            self.warm_start_articles(ids, donors=donors, window=donor_window)

    def _refuse_warm_start(self):
        if self._sharded() or hasattr(self.engine, "replica_update_items"):
            from .._lib import TcarError
            raise TcarError("warm start needs the whole catalog on one engine: it is not built for the catalog-sharded engine or the "
                            "data-parallel replicas")

    def warm_start_articles(self, ids, donors=16, window=None, min_sim=0.0, **kw):
        """Item rows for cold articles from their content neighbours, and nothing else (engine.TcarEngine.warm_start_items; it has the
        options: exclude, panel): ids int [U], 0-based; donors = the k of the neighbour lists; window = (lo, hi), ONE pair or one
        pair per article, in minutes since the earliest publish time (`minute_of(datetime)`): only articles published in [lo, hi)
        donate — the way to keep spare and retired rows, whose keys lie above every hi, out of the pool.  Returns the engine's
        WarmStart(rows, support, wsum, donors, sims) on the device.  The model keeps no item table of its own: the engine's is the one."""
        self._refuse_warm_start()
        if window is not None:
            self._item_keys()
        return self.engine.warm_start_items(ids, k=donors, min_sim=min_sim, window=window, **kw)

    def _sharded(self) -> bool:
        """is the engine the catalog-sharded one (its serving calls are collectives under names of their own)?"""
        return hasattr(self.engine, "shard_retrieve")

    def score_candidates(self, sessions, candidates, clicked=None, **kw):
        """Score and rank the items every session of `sessions` names — a feed dict as `recommend` takes it; candidates int [B, C],
        0-based ids, -1 = an empty slot — without touching the rest of the catalog: engine.CandResult(scores, rank_of, order, counts,
        metrics) on the device (engine.TcarEngine.score_candidates).  With clicked [B, C] (0 / 1) the counts and metrics of each
        list are those of an impression: host.metrics.impression_metrics turns them into AUC / MRR / nDCG@5 / nDCG@10.  With the
        catalog-sharded engine a COLLECTIVE (sharded.ShardedEngine.shard_score_candidates: cap=, T= and, without sessions, C=)."""
        call = self.engine.shard_score_candidates if self._sharded() else self.engine.score_candidates
        return call(self._feed(sessions), candidates, clicked, **kw)

    @staticmethod
    def _feed(sessions):
        """what recommend / retrieve / score_candidates take as `sessions`: a feed dict — rectangular, or a ragged one (flat rows +
        "len", host.data.ragged_arrays / pack_sessions) — or a LIST of rectangular feeds of any lengths, which becomes one ragged
        feed (sessions in list order, feed after feed): one call and one stream of the catalog for all of them"""
        if isinstance(sessions, (list, tuple)):
            return pack_sessions(sessions)
        return sessions
