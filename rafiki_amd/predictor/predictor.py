"""Predictor: top-k trained models resident on ONE GPU, dynamic batching, on-device ensembling.

Reference parity: rafiki/predictor/predictor.py (``Predictor.predict`` :31-74) + inference
workers (worker/inference.py:31-93) + Redis queues (cache/cache.py).  The reference fans every
query out through Redis lists to one container per model and polls for answers every 0.25 s
(≥0.25-0.5 s latency floor, ≤128 QPS per worker).  Here:
  * all top-k models live in this process on one MI355X (288 GB HBM holds thousands of such
    models); ``ParamCache`` accounts their bytes;
  * requests go through a lock-free-ish in-process queue into a dynamic batcher (up to
    ``max_batch`` queries or ``max_wait_ms``), replacing Redis + polling;
  * models exposing ``predict_proba(queries) -> Tensor[Q, C]`` (the native zoo: hipGraph-captured
    bucketed forwards) run on their own HIP streams and are ensembled by the gfx950
    ensemble-mean kernel; any other BaseModel falls back to ``predict()`` + host ensembling;
  * every request has a timeout (reference bug (g)); a model that fails is dropped from that
    batch's ensemble (partial-ensemble fallback) instead of hanging the request;
  * native ensembles run as ONE hipGraph per batch bucket (``ensemble_graph``: H2D, the k
    forwards on concurrent captured branches, the ensemble kernel, D2H);
  * replicas (reference INFERENCE_WORKER_REPLICAS_PER_TRIAL, config.py:10 / services_manager.py:
    53-87): R copies of the ensemble, spread over the predictor's GPUs, each with its own graphs,
    buffers and stream; every request runs on the least-busy replica, so concurrent requests (HTTP
    executor threads, the batcher) overlap instead of queueing behind one graph;
  * trials trained in this process are taken from HBM (``resident.STORE``) instead of re-read
    from their params files.
"""
from __future__ import annotations

import logging
import os
import pickle
import queue
import threading
import time
import traceback
from concurrent.futures import Future
from contextlib import contextmanager
from typing import List, Optional, Tuple

from .. import config
from ..constants import TaskType
from .ensemble import ensemble_predictions, ensemble_probabilities

logger = logging.getLogger(__name__)


class ParamCache:
    """Byte-budgeted registry of resident models (LRU eviction beyond the budget)."""

    def __init__(self, budget_bytes: float):
        self.budget = float(budget_bytes)
        self._items = {}
        self._order = []
        self._lock = threading.Lock()

    @staticmethod
    def model_bytes(model) -> int:
        fn = getattr(model, 'resident_bytes', None)
        return int(fn()) if callable(fn) else 0

    def put(self, key, model):
        with self._lock:
            self._items[key] = (model, self.model_bytes(model))
            if key in self._order:
                self._order.remove(key)
            self._order.append(key)
            evicted = []
            while self.used > self.budget and len(self._order) > 1:
                k = self._order.pop(0)
                evicted.append(self._items.pop(k)[0])
            return evicted

    def get(self, key):
        with self._lock:
            v = self._items.get(key)
            return None if v is None else v[0]

    @property
    def used(self):
        return sum(b for _, b in self._items.values())

    def keys(self):
        return list(self._order)


class RemoteWorkerModel:
    """Proxy for a model served by an ``InferenceWorker`` process (``workers`` serving mode)."""

    def __init__(self, worker_id, cache):
        self.worker_id = worker_id
        self.cache = cache

    def submit(self, ids, queries):
        self.cache.add_queries_of_worker(self.worker_id, list(zip(ids, queries)))

    def collect(self, ids, deadline):
        from ..cache.cache import MISSING
        out = []
        for i in ids:
            while True:
                left_ms = int((deadline - time.perf_counter()) * 1000)
                p = self.cache.pop_prediction_of_worker(self.worker_id, i, timeout_ms=max(0, min(left_ms, 200)))
                if p is not MISSING or left_ms <= 0:
                    break
            if p is MISSING:
                raise TimeoutError('worker {} did not answer in time'.format(self.worker_id))
            out.append(p)
        return out


class _Replica:
    """One copy of the ensemble: its models, HIP streams and (lazily) its ensemble graphs."""

    def __init__(self, idx, models):
        self.idx = idx
        self.models = list(models)
        self.inflight = 0
        self.served = 0
        self.streams = None
        self.graphs = None
        self.graphs_failed = False
        # the per-model path writes each model's static bucket buffers and replays its graphs:
        # two threads on one replica must not interleave there (the ensemble graph has its own lock)
        self.lock = threading.RLock()


class Predictor:
    def __init__(self, models: Optional[List[Tuple[str, object]]] = None, task=TaskType.IMAGE_CLASSIFICATION,
                 max_batch: int = 256, max_wait_ms: float = 2.0, timeout_s: float = None,
                 weights: Optional[List[float]] = None, replicas: Optional[List[List[Tuple[str, object]]]] = None):
        """models: replica 0's [(trial id, model)]; replicas: further copies of the same ensemble
        (same trial order), e.g. on other GPUs."""
        self.task = task
        self.models = list(models or [])
        self.max_batch = max_batch
        self.max_wait_s = max_wait_ms / 1000.0
        self.timeout_s = timeout_s or config.PREDICTOR_TIMEOUT_S
        self.weights = weights
        self.replicas = [_Replica(0, self.models)] + [_Replica(i + 1, r) for i, r in enumerate(replicas or [])]
        for r in self.replicas[1:]:
            if [n for n, _ in r.models] != [n for n, _ in self.models]:
                raise ValueError('every replica must hold the same trials in the same order')
        self._rlock = threading.Lock()
        self.cache = ParamCache(config.get_config().node.param_cache_gb * 1e9)
        for r in self.replicas:
            for name, m in r.models:
                self.cache.put((name, r.idx), m)
        self._q: "queue.Queue" = queue.Queue()
        self._threads = []
        self._stop = threading.Event()
        self.stats = {'batches': 0, 'queries': 0, 'errors': 0}

    @contextmanager
    def _replica(self):
        """The least-busy replica for the duration of one request."""
        with self._rlock:
            r = min(self.replicas, key=lambda x: (x.inflight, x.served))
            r.inflight += 1
        try:
            yield r
        finally:
            with self._rlock:
                r.inflight -= 1
                r.served += 1

    def _ensemble_graphs(self, r):
        """The replica's one-graph-per-bucket ensemble, when its models support it."""
        if r.graphs is not None or r.graphs_failed or os.environ.get('RAFIKI_ENSEMBLE_GRAPH', '1') == '0':
            return r.graphs
        from . import ensemble_graph as EG
        from ..ops.graphs import quiesced
        # Built once per replica, under the process-wide capture lock.  Requests share a replica, so two threads can
        # meet it fresh: unlocked, each built an EnsembleGraphs, the second assignment dropped the first one's
        # captured graphs, and their destructors (and the construction's allocations) ran while another replica's
        # thread was capturing — which aborts the process (ops/graphs.py).
        with quiesced():
            if r.graphs is None and not r.graphs_failed:
                if EG.supports([m for _, m in r.models]):
                    r.graphs = EG.EnsembleGraphs([m for _, m in r.models], self.weights)
                else:
                    r.graphs_failed = True
        return r.graphs

    def _graph_call(self, r, fn):
        """Run fn(graphs) on the replica's ensemble graph; None when unavailable or it failed (the
        replica then stays on the per-model path)."""
        g = self._ensemble_graphs(r)
        if g is None:
            return None
        try:
            return fn(g)
        except Exception:
            logger.error('ensemble graph failed on replica %d, using per-model path:\n%s', r.idx,
                         traceback.format_exc())
            r.graphs, r.graphs_failed = None, True
            return None

    # ------------------------------------------------------------------ loading from the DB
    @classmethod
    def from_inference_job(cls, inference_job_id, db=None, replicas=None, devices=None, **kw):
        """Load the job's top-k trials.  ``replicas`` (default INFERENCE_WORKER_REPLICAS_PER_TRIAL,
        capped at one per device unless that variable or ``replicas`` is given explicitly) copies go
        round-robin over ``devices`` (default: every GPU visible to this process).  A
        trial trained in this process is taken from HBM (resident.STORE) for replica 0 on its own
        GPU; everything else is read from the params file once and instantiated per replica."""
        if os.environ.get('RAFIKI_INFERENCE_MODE', 'local') == 'workers':
            return cls.from_inference_workers(inference_job_id, db=db, **kw)
        from ..db.database import Database
        from ..model.model import load_model_class
        from ..parallel.context import TrialContext, current, use_context
        from .resident import STORE
        db = db or Database()
        ij = db.get_inference_job(inference_job_id)
        tj = db.get_train_job(ij.train_job_id)
        n_rep = max(1, int(replicas if replicas is not None else config.INFERENCE_WORKER_REPLICAS_PER_TRIAL))
        if devices is None:
            devices = _serving_devices()
        if replicas is None and 'INFERENCE_WORKER_REPLICAS_PER_TRIAL' not in os.environ:
            # the default is at most one replica per GPU: two replicas sharing one GPU serve 0.71x of one
            # (profiles/predictor_qps_r4_2replicas.json); an explicit count is honoured as given
            n_rep = min(n_rep, max(1, len(devices)))
        sets = [[] for _ in range(n_rep)]
        for w in db.get_workers_of_inference_job(inference_job_id):
            trial = db.get_trial(w.trial_id)
            sub = db.get_sub_train_job(trial.sub_train_job_id)
            mrec = db.get_model(sub.model_id)
            clazz = load_model_class(mrec.model_file_bytes, mrec.model_class)
            params = None
            for r in range(n_rep):
                dev = devices[r % len(devices)]
                inst = STORE.take(trial.id) if r == 0 else None
                if inst is not None and str(getattr(inst, 'device', '')) != str(dev):
                    STORE.offer(trial.id, inst, float(trial.score or 0.0))   # trained on another GPU
                    inst = None
                if inst is None:
                    if params is None:
                        with open(trial.params_file_path, 'rb') as f:
                            params = pickle.loads(f.read())
                    ctx = TrialContext(device=dev) if dev is not None else current()
                    with use_context(ctx):
                        inst = clazz(**(trial.knobs or {}))
                        inst.load_parameters(params)
                sets[r].append((trial.id, inst))
        return cls(sets[0], task=tj.task, replicas=sets[1:], **kw)

    @classmethod
    def from_inference_workers(cls, inference_job_id, db=None, cache=None, **kw):
        from ..cache import Cache
        from ..db.database import Database
        db = db or Database()
        ij = db.get_inference_job(inference_job_id)
        tj = db.get_train_job(ij.train_job_id)
        cache = cache or Cache()
        models = [(w.trial_id, RemoteWorkerModel(w.service_id, cache))
                  for w in db.get_workers_of_inference_job(inference_job_id)]
        return cls(models, task=tj.task, **kw)

    # ------------------------------------------------------------------------- inference
    def _fast_path(self):
        return self.task == TaskType.IMAGE_CLASSIFICATION and self.models and all(
            callable(getattr(m, 'predict_proba', None)) for _, m in self.models)

    def predict(self, queries):
        """Synchronous batched prediction over the whole ensemble."""
        if not queries:
            return []
        if self.models and all(isinstance(m, RemoteWorkerModel) for _, m in self.models):
            return self._predict_remote(queries)
        if self._fast_path():
            try:
                return self._predict_fast(queries)
            except Exception:
                logger.error('fast path failed, falling back:\n%s', traceback.format_exc())
        with self._replica() as r:
            return self._predict_models(r, queries)

    def _predict_models(self, r, queries):
        with r.lock:
            return self._predict_models_locked(r, queries)

    def _predict_models_locked(self, r, queries):
        preds, ok = [], []
        for name, m in r.models:
            try:
                preds.append(m.predict(queries))
                ok.append(name)
            except Exception:
                self.stats['errors'] += 1
                logger.error('model %s failed:\n%s', name, traceback.format_exc())
        if not preds:
            raise RuntimeError('every model of the ensemble failed')
        return ensemble_predictions(preds, self.task)

    def predict_array(self, arr):
        """Ensemble probabilities for a numpy batch (images already decoded): skips the per-query
        list handling of ``predict``; native models take the uint8 batch straight to the device."""
        if self._fast_path():
            import numpy as np
            import torch
            with self._replica() as r:
                dev = _cuda_device_of(r.models)
                if dev is not None and all(callable(getattr(m, 'input_signature', None)) for _, m in r.models):
                    host = _decode_once(r.models, arr)
                    self.stats['queries'] += len(arr)
                    out = self._graph_call(r, lambda g: g.run_host(host))
                    if out is not None:
                        return out
                    inputs = {s: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True) for s, a in host.items()}
                    return self._proba_device_on(r, inputs).cpu().numpy()
        return self.predict(arr.tolist())

    def staged_graphs(self, idx):
        """(replica, its ensemble graphs, the image shape they take) for replica ``idx`` — what the native
        front end's double-buffered batch loop drives directly — or None when that replica has no
        one-graph ensemble or takes several input signatures."""
        if not self._fast_path() or idx >= len(self.replicas):
            return None
        r = self.replicas[idx]
        if not all(callable(getattr(m, 'input_signature', None)) for _, m in r.models):
            return None
        g = self._ensemble_graphs(r)
        if g is None or len(g.sigs) != 1:
            return None
        sig = g.sigs[0]
        if not (isinstance(sig, tuple) and len(sig) == 3 and sig[0] == 'image_u8'):
            return None
        size, ch = int(sig[1]), int(sig[2])
        return r, g, ((size, size) if ch == 1 else (size, size, ch))

    def _predict_remote(self, queries):
        """Fan the batch out to every worker first, then gather (workers run concurrently); a worker
        that misses the deadline is dropped from this batch's ensemble (partial-ensemble fallback)."""
        import uuid
        base = uuid.uuid4().hex[:12]
        ids = ['{}-{}'.format(base, i) for i in range(len(queries))]
        for _, m in self.models:
            m.submit(ids, queries)
        deadline = time.perf_counter() + self.timeout_s
        preds = []
        for name, m in self.models:
            try:
                p = m.collect(ids, deadline)
                if any(x is None for x in p):
                    raise RuntimeError('worker {} failed to predict'.format(name))
                preds.append(p)
            except Exception:
                self.stats['errors'] += 1
                logger.error('remote model %s dropped from ensemble:\n%s', name, traceback.format_exc())
        if not preds:
            raise RuntimeError('every model of the ensemble failed')
        return ensemble_predictions(preds, self.task)

    def _predict_fast(self, queries):
        return self.predict_proba(queries).cpu().tolist()

    def predict_proba(self, queries):
        """Ensemble probabilities [Q, C] as a tensor (on the GPU when the models are).

        Queries are decoded to uint8 once per distinct model input signature and uploaded once
        (pinned, non-blocking); every model then runs its hipGraph-captured bucketed forward on its
        own HIP stream, and the gfx950 ensemble-mean kernel reduces the [models, Q, C] stack."""
        import torch
        with self._replica() as r:
            dev = _cuda_device_of(r.models)
            if dev is None:
                probs = [m.predict_proba(queries) for _, m in r.models]
                return ensemble_probabilities(torch.stack([p.float().cpu() for p in probs]))
            host = _decode_once(r.models, queries)
            if len(host) and all(callable(getattr(m, 'input_signature', None)) for _, m in r.models):
                out = self._graph_call(r, lambda g: g.run_host(host))
                if out is not None:
                    return torch.from_numpy(out)
            inputs = {s: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True) for s, a in host.items()}
            return self._proba_device_on(r, inputs, queries)

    def predict_proba_device(self, inputs, queries=None):
        """inputs: {input_signature: device uint8 batch} -> device probabilities.  Models without
        a signature get ``queries``."""
        with self._replica() as r:
            if queries is None and inputs and all(callable(getattr(m, 'input_signature', None)) for _, m in r.models):
                out = self._graph_call(r, lambda g: g.run_device(inputs))
                if out is not None:
                    return out
            return self._proba_device_on(r, inputs, queries)

    def _proba_device_on(self, r, inputs, queries=None):
        """Per-model path: each model's bucketed graph on its own HIP stream, then the ensemble kernel."""
        with r.lock:
            return self._proba_device_on_locked(r, inputs, queries)

    def _proba_device_on_locked(self, r, inputs, queries=None):
        import torch
        dev = next(iter(inputs.values())).device if inputs else torch.device('cuda')
        if r.streams is None or len(r.streams) != len(r.models):
            r.streams = [torch.cuda.Stream(device=dev) for _ in r.models]
        main = torch.cuda.current_stream(dev)
        outs = []
        for (name, m), s in zip(r.models, r.streams):
            s.wait_stream(main)
            with torch.cuda.stream(s):
                sig_fn = getattr(m, 'input_signature', None)
                sig = sig_fn() if callable(sig_fn) else None
                if sig is not None and sig in inputs:
                    p = m.predict_proba_images(inputs[sig])
                else:
                    p = m.predict_proba(queries)
                outs.append(p)
        for s in r.streams:
            main.wait_stream(s)
        for p in outs:
            p.record_stream(main)
        stacked = torch.stack(outs)
        w = None
        if self.weights is not None:
            w = torch.tensor(self.weights, dtype=torch.float32, device=dev)
        return ensemble_probabilities(stacked, w)

    # ------------------------------------------------------------------- dynamic batching
    def start(self):
        """One batching consumer per replica over the shared request queue (the reference's
        replicas each pop from the same Redis queue).  For native image ensembles each consumer is
        a two-stage pipeline: a collector thread batches and decodes queries (nested lists -> uint8)
        while the device thread runs the previous batch's hipGraph, through a 2-deep hand-off."""
        if not self._threads:
            self._stop.clear()
            for i, r in enumerate(self.replicas):
                if self._pipelined(r):
                    hand = queue.Queue(maxsize=2)
                    for fn, nm in ((self._collect_loop, 'collect'), (self._device_loop, 'device')):
                        t = threading.Thread(target=fn, args=(r, hand), name='rafiki-batcher-{}-{}'.format(nm, i),
                                             daemon=True)
                        t.start()
                        self._threads.append(t)
                    continue
                t = threading.Thread(target=self._batch_loop, name='rafiki-batcher-{}'.format(i), daemon=True)
                t.start()
                self._threads.append(t)
        return self

    def _pipelined(self, r):
        from . import ensemble_graph as EG
        return (self._fast_path() and os.environ.get('RAFIKI_BATCHER_PIPELINE', '1') != '0'
                and all(callable(getattr(m, 'input_signature', None)) for _, m in r.models)
                and EG.supports([m for _, m in r.models]))

    def _take_batch(self):
        try:
            first = self._q.get(timeout=0.05)
        except queue.Empty:
            return None
        batch = [first]
        deadline = time.perf_counter() + self.max_wait_s
        while len(batch) < self.max_batch:
            rem = deadline - time.perf_counter()
            try:
                batch.append(self._q.get(timeout=max(0.0, rem)) if rem > 0 else self._q.get_nowait())
            except queue.Empty:
                break
        return batch

    def _collect_loop(self, r, hand):
        while not self._stop.is_set():
            batch = self._take_batch()
            if batch is None:
                continue
            futs = [f for _, f in batch]
            try:
                host = _decode_once(r.models, [q for q, _ in batch])
            except Exception as e:
                for f in futs:
                    f.set_exception(e)
                continue
            while not self._stop.is_set():
                try:
                    hand.put((host, futs), timeout=0.05)
                    break
                except queue.Full:
                    continue

    def _device_loop(self, r, hand):
        while not self._stop.is_set():
            try:
                host, futs = hand.get(timeout=0.05)
            except queue.Empty:
                continue
            with self._rlock:
                r.inflight += 1
            try:
                out = self._graph_call(r, lambda g: g.run_host(host))
                if out is None:
                    import torch
                    dev = _cuda_device_of(r.models)
                    inputs = {s: torch.from_numpy(a).to(dev) for s, a in host.items()}
                    out = self._proba_device_on(r, inputs).cpu().numpy()
                rows = out.tolist()
                for f, p in zip(futs, rows):
                    f.set_result(p)
            except Exception as e:
                for f in futs:
                    if not f.done():
                        f.set_exception(e)
            finally:
                with self._rlock:
                    r.inflight -= 1
                    r.served += 1
            self.stats['batches'] += 1
            self.stats['queries'] += len(futs)

    def stop(self):
        self._stop.set()
        for t in self._threads:
            t.join(timeout=5)
        self._threads = []

    def submit(self, query) -> Future:
        fut = Future()
        self._q.put((query, fut))
        if not self._threads:
            self.start()
        return fut

    def predict_one(self, query):
        return self.submit(query).result(timeout=self.timeout_s)

    def _batch_loop(self):
        while not self._stop.is_set():
            try:
                first = self._q.get(timeout=0.05)
            except queue.Empty:
                continue
            batch = [first]
            deadline = time.perf_counter() + self.max_wait_s
            while len(batch) < self.max_batch:
                rem = deadline - time.perf_counter()
                try:
                    batch.append(self._q.get(timeout=max(0.0, rem)) if rem > 0 else self._q.get_nowait())
                except queue.Empty:
                    break
            queries = [q for q, _ in batch]
            try:
                preds = self.predict(queries)
                for (_, fut), p in zip(batch, preds):
                    fut.set_result(p)
            except Exception as e:
                for _, fut in batch:
                    fut.set_exception(e)
            self.stats['batches'] += 1
            self.stats['queries'] += len(batch)


def _cuda_device_of(models):
    import torch
    for _, m in models:
        d = getattr(m, 'device', None)
        if d is not None and torch.device(d).type == 'cuda':
            return torch.device(d)
    return None


def _decode_once(models, queries):
    """{input signature: contiguous uint8 numpy batch}: queries decoded once per distinct model
    input signature, not once per model."""
    import numpy as np
    out = {}
    for _, m in models:
        sig_fn = getattr(m, 'input_signature', None)
        sig = sig_fn() if callable(sig_fn) else None
        if sig is not None and sig not in out:
            out[sig] = np.ascontiguousarray(m.queries_to_images(queries))
    return out


def _serving_devices():
    """GPUs this predictor serves from: RAFIKI_PREDICTOR_DEVICES ("0,1") or every visible GPU;
    [None] (the current context's device) on a host without GPUs."""
    import torch
    env = os.environ.get('RAFIKI_PREDICTOR_DEVICES', '')
    if env:
        return [torch.device('cuda', int(v)) for v in env.split(',') if v.strip()]
    try:
        n = torch.cuda.device_count() if torch.cuda.is_available() else 0
    except Exception:
        n = 0
    return [torch.device('cuda', i) for i in range(n)] or [None]
