"""Reconstruction negatives on the device, drawn by word frequency as the reference's sampler draws them
(cliora/blocks/negative_sampler.py, called per batch from data/batch_iterator.py:158-168).

The reference counts the corpus with a ``Counter``, turns the counts into ``freq**0.75 + 1e-2 / V`` normalised, and draws every
batch's ``k_neg`` ids on the host with ``RandomState.choice(V, k, p=dist, replace=False)``.  Here the counts are one launch
(include/cliora_chart.h: cliora_token_counts) and a draw is the exponential race of cliora_neg_sample, the same law as numpy's
successive sampling, on the current stream with a counter-based generator: no host work and no copy per batch.

    from cliora_amd.sampling import calculate_freq_dist, NegativeSampler
    freq = calculate_freq_dist(dset['sentences'], len(word2idx), 'cuda')
    sampler = NegativeSampler(freq, options.freq_dist_power, seed=options.seed, stream_id=rank)
    trainer = harness.Trainer(net, lr, negative_sampler=sampler, k_neg=options.k_neg)

Deliberate difference: the reference normalises with a float32 ``sum`` and numpy then rejects the vector at large V ("probabilities
do not sum to 1", seen at V = 400k).  The draw here does not depend on the scale of the weights, so nothing is normalised for it and
there is no such failure; ``.dist`` is normalised with a float64 sum.
"""
import ctypes as C
import itertools
import os

import numpy as np
import torch

from . import _lib
from ._lib import ptr_or_null as _p, stream as _stream

MAX_K = 1024


def _flat_ids(data):
    if isinstance(data, torch.Tensor):
        if data.dim() != 1:
            raise ValueError('token ids: a 1-D tensor or a list of id sequences, not a %d-D tensor' % data.dim())
        return data.to(torch.int64)
    if isinstance(data, np.ndarray) and data.ndim == 1:
        return torch.from_numpy(data.astype(np.int64, copy=False))
    flat = np.fromiter(itertools.chain.from_iterable(data), dtype=np.int64)         # the one host flatten
    return torch.from_numpy(flat)


def token_counts(ids, vocab_size):
    """cliora_token_counts: (V,) fp32 counts of a 1-D int64 CUDA tensor of ids; raises on ids outside [0, V)."""
    if vocab_size < 1:
        raise ValueError('vocab_size = %d must be positive' % vocab_size)
    dev = ids.device
    with torch.cuda.device(dev):
        ids = ids.contiguous()
        counts = torch.empty(vocab_size, dtype=torch.float32, device=dev)
        bad = torch.empty((), dtype=torch.int64, device=dev)
        _lib.call('cliora_token_counts', ids.numel(), _p(ids), vocab_size, _p(counts), _p(bad), _stream())
        n_bad = int(bad)
    if n_bad:
        raise ValueError('%d token id(s) outside [0, %d): the vocabulary does not cover the corpus' % (n_bad, vocab_size))
    return counts


def calculate_freq_dist(sentences, vocab_size, device='cuda'):
    """negative_sampler.py:15-24: the float32 count of every id of the corpus, on `device`.  `sentences`: a list of id sequences
    (dset['sentences']) or a 1-D tensor of ids.  One host flatten, one host-to-device copy, one count launch."""
    ids = _flat_ids(sentences)
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if ids.device != device:
        ids = ids.to(device, non_blocking=False)
    return token_counts(ids, vocab_size)


class NegativeSampler(object):
    """negative_sampler.py:27-37 on the device.  ``.dist``: the normalised float32 distribution; ``.sample(k)``: (k,) int64 ids on the
    current stream; ``.sample_many(S, k)``: (S, k) in one call.  Every draw takes the next value of a draw counter, which
    ``set_seed`` resets, so a seeded sampler's draws are a function of (seed, stream_id, draw number).  seed=None seeds from
    os.urandom, as the reference's unseeded RandomState().  Ranks of a data-parallel run: stream_id=rank gives independent draws per
    rank (the reference's unseeded per-process samplers), one stream_id on every rank gives the same draws everywhere."""

    def __init__(self, freq_dist, dist_power, epsilon=10 ** -2, seed=None, stream_id=0):
        f = freq_dist if isinstance(freq_dist, torch.Tensor) else torch.from_numpy(np.asarray(freq_dist, dtype=np.float32))
        if not f.is_cuda:
            f = f.cuda()
        f = f.to(torch.float32).contiguous()
        if f.dim() != 1 or f.numel() < 1:
            raise ValueError('freq_dist must be a non-empty vector')
        self.V = f.numel()
        self.device = f.device
        self.weights = f.pow(dist_power) + np.float32(epsilon * (1 / self.V))          # the race's weights: any scale will do
        self.dist = (self.weights.double() / self.weights.double().sum()).float()
        self.n_positive = int((self.weights > 0).sum())
        if not bool(torch.isfinite(self.weights).all()):
            raise ValueError('negative sampler: the weights freq_dist**power + epsilon / V are not all finite')
        self.stream_id = int(stream_id)
        self._ws = None
        self.set_seed(int.from_bytes(os.urandom(8), 'little') if seed is None else seed)

    def set_seed(self, seed):
        self.seed = int(seed) & (2 ** 64 - 1)
        self.draws = 0

    def _draw(self, S, k, keys=False, offset=None):
        if not 1 <= k <= MAX_K:
            raise ValueError('k = %d: the device sampler supports 1 <= k <= %d' % (k, MAX_K))
        if k > self.n_positive:
            raise ValueError('Fewer non-zero entries in p than size')
        off = self.draws if offset is None else offset
        with torch.cuda.device(self.device):
            ids = torch.empty((S, k), dtype=torch.int64, device=self.device)
            E = torch.empty((S, k), dtype=torch.float64, device=self.device) if keys else None
            nbytes = _lib.fn('cliora_neg_sample_workspace_bytes')(self.V, S, k)
            if nbytes and (self._ws is None or self._ws.numel() < nbytes):
                self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            ws = self._ws if nbytes else None
            _lib.call('cliora_neg_sample', self.V, _p(self.weights), self.n_positive, S, k, C.c_uint64(self.seed), C.c_uint64(off),
                      C.c_uint32(self.stream_id), _p(ids), _p(E), _p(ws), nbytes, _stream())
        if offset is None:
            self.draws += S
        return (ids, E) if keys else ids

    def sample(self, num_samples):
        return self._draw(1, num_samples)[0]

    def sample_many(self, S, num_samples):
        return self._draw(S, num_samples)

    def sample_with_keys(self, S, num_samples, offset=None):
        """(ids, E): the draws and their race keys (float64), for tests; offset: draw number of the first row (default: the counter's,
        which then advances)."""
        return self._draw(S, num_samples, keys=True, offset=offset)


def choose_negative_samples(negative_sampler, k_neg):
    """negative_sampler.py:9-12: one draw of k_neg ids, already on the device."""
    return negative_sampler.sample(k_neg)
