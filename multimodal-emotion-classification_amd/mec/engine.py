"""Batched tensor API over the C ABI: device-resident inputs in, device tensors out.

Torch owns device memory and the stream (plumbing); all arithmetic runs in the HIP
kernels of libmec_hip.so. Each call validates shapes/dtypes/devices on the host before
any launch, and raises MecError when the library or a GPU is unavailable — there is no
CPU fallback on this path.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np
import torch

from . import _lib, image as _image, jpeg as _jpeg, synthetic, tokenize as _tok, wav as _wav
from ._lib import MecError

TAG_BERT_FFN2 = 5  # launch class of BERT's FFN2 GEMM (mec_common.h Tag)
TAG_BERT_QKV = 1  # ... and of its QKV GEMM
TAG_BERT_OPROJ = 3  # ... and of its attention output projection

KINDS = synthetic.KIND_IDS


def _ptr(t: torch.Tensor | None):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device: torch.device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check_tensor(name, t, dtype, shape, device):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f'{name}: expected a torch.Tensor, got {type(t).__name__}')
    if t.device != device:
        raise ValueError(f'{name}: on {t.device}, expected {device}')
    if t.dtype != dtype:
        raise TypeError(f'{name}: dtype {t.dtype}, expected {dtype}')
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name}: shape {tuple(t.shape)}, expected {tuple(shape)}')
    if not t.is_contiguous():
        raise ValueError(f'{name}: must be contiguous')


def require_gpu(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise MecError('no ROCm GPU visible: the HIP inference path has no CPU fallback')
    if device is None:
        return torch.device('cuda', torch.cuda.current_device())
    d = torch.device(device)
    if d.type != 'cuda':
        raise MecError(f'device {d}: the HIP inference path runs on a ROCm GPU only')
    return torch.device('cuda', d.index if d.index is not None else torch.cuda.current_device())


class HipModel:
    """Owns one mec_model handle (packed device weights + workspace).

    fp32x3 handles answer on data outside their activation-plane envelope instead of failing: the
    checked paths (`checked`, and through it the drop-in classes and FusedPipeline.check) notice a
    raised range flag (mec_model_check == MEC_ERR_X3_RANGE), re-run the batch on an fp32 handle of the
    same weights (`fp32_twin`, the exact-fp32 HIP engine, created on first use) and re-create this
    handle with 8 more binades of plane headroom (`x3_headroom`), so later batches run fp32x3 again."""

    kind: str = ''
    X3_HEADROOM_STEP = 8  # binades added per range trip (mec_create_opt "x3_headroom", at most 24)

    def __init__(self, weights=None, seed: int = 1234, device=None, precision: str = 'f16', opts=None):
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}, got {precision!r}")
        self.lib = _lib.load()
        self.device = require_gpu(device)
        self.precision = precision
        # the weights dict (synthetic weights are cached per (kind, seed), so this holds no copy): a range
        # trip re-creates the handle from it
        self._w = weights if weights is not None else synthetic.weights(self.kind, seed)
        self._seed = seed
        self._copts = dict(opts or {})  # creation-time knobs (mec_create_opt)
        self._knobs = []                # set_option calls, replayed onto a re-created handle
        self._twin = None
        self._x3_cal = None             # observed maxima of a calibrated image handle (ImageEncoder.calibrate)
        self.x3_reruns = 0              # batches re-run on the fp32 engine after a range trip
        self._lock = threading.Lock()
        self.handle = None
        self.handle = self._create(self._copts)

    def _create(self, copts):
        blob = synthetic.pack(self.kind, self._w)
        want = self.lib.mec_blob_size(KINDS[self.kind])
        if blob.size != want:
            raise MecError(f'{self.kind}: blob has {blob.size} floats, library expects {want}')
        h = ctypes.c_void_p()
        torch.cuda.set_device(self.device)
        spec = ','.join(f'{k}={int(v)}' for k, v in copts.items()).encode()
        if self._x3_cal is not None:  # a calibrated fp32x3 handle: the observed maxima set the plane exponents
            cal = np.ascontiguousarray(self._x3_cal, np.float32)
            _lib.check(self.lib.mec_create_x3_calibrated(KINDS[self.kind], blob.ctypes.data_as(_lib.c_fp), blob.size,
                                                         self.device.index, spec, cal.ctypes.data_as(_lib.c_fp),
                                                         int(cal.size), ctypes.byref(h)),
                       f'mec_create_x3_calibrated({self.kind})')
            return h
        _lib.check(self.lib.mec_create_opt(KINDS[self.kind], blob.ctypes.data_as(_lib.c_fp), blob.size,
                                           self.device.index, _lib.PRECISIONS[self.precision], spec, ctypes.byref(h)),
                   f'mec_create({self.kind}, {self.precision})')
        return h

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.mec_destroy(self.handle)
            self.handle = None
        if getattr(self, '_twin', None) is not None:
            self._twin.close()
            self._twin = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key: str, value: int):
        """One tuning knob of THIS handle (mec_model_set_option; include/mec.h lists them)."""
        _lib.check(self.lib.mec_model_set_option(self.handle, key.encode(), int(value)), f'set_option({key}={value})')
        self._knobs.append((key, int(value)))

    def check(self):
        """Raise MecError if a kernel of this handle flagged an error after the fact since the
        last check (mec_model_check; speech: an expired hand-off wait, whose forward's probs are
        NaN; fp32x3: X3RangeError, an activation outside the planes' range). Call once the stream
        that ran the forwards has been synchronized."""
        _lib.check(self.lib.mec_model_check(self.handle), f'{self.kind} forward')

    def x3_report(self) -> str:
        """The activation-plane exponents this fp32x3 handle was created with (mec_model_x3_report)."""
        r = self.lib.mec_model_x3_report(self.handle)
        return r.decode() if r else ''

    @property
    def x3_headroom(self) -> int:
        return int(self._copts.get('x3_headroom', 0))

    def fp32_twin(self):
        """An exact-fp32 handle of the same kind and weights (created on first use)."""
        if self._twin is None:
            self._twin = type(self)(self._w, self._seed, self.device, 'fp32')
        return self._twin

    def x3_widen(self):
        """Re-create this fp32x3 handle with X3_HEADROOM_STEP more binades of plane headroom (a calibrated
        handle keeps its observed bounds: the headroom applies on top of them)."""
        hr = min(24, self.x3_headroom + self.X3_HEADROOM_STEP)
        if hr == self.x3_headroom:
            return
        self._recreate(dict(self._copts, x3_headroom=hr))

    def _recreate(self, copts):
        """Replace the handle by one created with `copts` (and the calibration held), the knobs replayed."""
        with self._lock:
            torch.cuda.synchronize(self.device)  # nothing of the old handle may still run
            h = self._create(copts)
            old, self.handle, self._copts = self.handle, h, copts
            self.lib.mec_destroy(old)
            for k, v in self._knobs:
                _lib.check(self.lib.mec_model_set_option(self.handle, k.encode(), v), f'set_option({k}={v})')

    def recover(self, method: str, args, outs):
        """After a synchronized forward `getattr(self, method)(*args)` -> `outs`: check the handle; on an
        fp32x3 range trip re-run the call on the fp32 twin, copy its results into `outs` (in place), widen
        this handle, and return True. Other errors raise as `check` does."""
        rc = self.lib.mec_model_check(self.handle)
        if rc == 0:
            return False
        if rc != _lib.ERR_X3_RANGE or self.precision != 'fp32x3':
            _lib.check(rc, f'{self.kind} forward')
        twin = self.fp32_twin()
        with torch.cuda.device(self.device):
            res = getattr(twin, method)(*args)
            for o, r in zip(outs, res):
                o.copy_(r)
            torch.cuda.synchronize(self.device)
        twin.check()
        self.x3_reruns += 1
        self.x3_widen()
        return True

    def checked(self, method: str, *args):
        """`getattr(self, method)(*args)`, synchronized and checked: an fp32x3 range trip is answered by
        the fp32 engine (recover) instead of raising. Returns the forward's outputs."""
        outs = getattr(self, method)(*args)
        torch.cuda.synchronize(self.device)
        self.recover(method, args, outs)
        return outs

    def gemm_tile(self, M: int, N: int, K: int, amode: int = 0) -> int:
        """The tile this handle's autotuner chose for a GEMM shape it has run (0 = not seen)."""
        return self.lib.mec_model_gemm_query(self.handle, amode, M, N, K)

    # hipEvent timing hook
    def prof_enable(self, tag: str | int):
        t = _lib.TAGS[tag] if isinstance(tag, str) else int(tag)
        _lib.check(self.lib.mec_prof_enable(self.handle, t), 'mec_prof_enable')

    def prof_read(self):
        ms = ctypes.c_double()
        n = ctypes.c_int()
        _lib.check(self.lib.mec_prof_read(self.handle, ctypes.byref(ms), ctypes.byref(n)), 'mec_prof_read')
        return ms.value, n.value

    def _empty(self, *shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.device)


class SpeechEncoder(HipModel):
    kind = 'speech'

    def forward(self, x: torch.Tensor):
        """x f32 [B,56] raw features -> (feat [B,64], logits [B,7], probs [B,7])."""
        B = x.shape[0] if x.dim() == 2 else -1
        _check_tensor('x', x, torch.float32, (B, 56), self.device)
        feat, logits, probs = self._empty(B, 64), self._empty(B, 7), self._empty(B, 7)
        with self._lock:
            _lib.check(self.lib.mec_speech_fwd(self.handle, _ptr(x), B, _ptr(feat), _ptr(logits), _ptr(probs),
                                               _stream(self.device)), 'mec_speech_fwd')
        return feat, logits, probs


class TextEncoder(HipModel):
    kind = 'text'

    VOCAB = 30522  # bert-base-uncased word embeddings

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        # BERT's GEMMs walk their tiles in groups of 4 M panels per XCD (the handle default is 8, which
        # ResNet50 keeps): fp32x3 fused step 25.51 -> 25.35 and 25.38 -> 25.31 ms, BERT alone 17.44 ->
        # 17.32 ms, f16 fused step 10.76 -> 10.74 ms; the same bits (profiles/r05y_ab_groupm_*.txt,
        # profiles/r05z_ab_groupm_*.txt)
        self.set_option('gemm_glds_group_m', 4)

    def forward(self, ids: torch.Tensor, mask: torch.Tensor, check_ids: bool = False):
        """ids/mask int32 [B,128] -> (cls [B,768], logits [B,7], probs [B,7]).

        check_ids: raise ValueError for ids outside [0, 30522) like nn.Embedding does (one
        device min/max reduction and a host sync; the batched hot path skips it, and the kernel
        then clamps out-of-range ids)."""
        if ids.dim() != 2:
            raise ValueError('ids: expected [B, L]')
        B, L = ids.shape
        if L != 128:
            raise ValueError('ids: L must be 128 (padding=max_length, Config.MAX_TEXT_LENGTH)')
        _check_tensor('ids', ids, torch.int32, (B, L), self.device)
        _check_tensor('mask', mask, torch.int32, (B, L), self.device)
        if check_ids and B:
            lo, hi = (int(v) for v in torch.aminmax(ids))
            if lo < 0 or hi >= self.VOCAB:
                raise ValueError(f'ids: token id out of range [0, {self.VOCAB}): min {lo}, max {hi}')
        cls, logits, probs = self._empty(B, 768), self._empty(B, 7), self._empty(B, 7)
        with self._lock:
            _lib.check(self.lib.mec_text_fwd(self.handle, _ptr(ids), _ptr(mask), B, L, _ptr(cls), _ptr(logits),
                                             _ptr(probs), _stream(self.device)), 'mec_text_fwd')
        return cls, logits, probs

    packed_rows = 0  # Bp of the last forward_packed plan

    def pack_plan(self, lens):
        """The first-fit-decreasing plan of mec_text_pack_plan for host lengths `lens` (each in [1,128])
        -> (row int32 [B], off int32 [B], Bp). Host only."""
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if lens.ndim != 1:
            raise ValueError('lens: expected a 1-d array of B lengths')
        if lens.size and (int(lens.min()) < 1 or int(lens.max()) > 128):
            raise ValueError(f'lens: every length must be in [1,128], got min {int(lens.min())}, max {int(lens.max())}')
        row, off = np.zeros(lens.size, np.int32), np.zeros(lens.size, np.int32)
        ip = ctypes.POINTER(ctypes.c_int32)
        bp = self.lib.mec_text_pack_plan(lens.ctypes.data_as(ip), int(lens.size), row.ctypes.data_as(ip),
                                         off.ctypes.data_as(ip))
        if bp < 0:
            _lib.check(bp, 'mec_text_pack_plan')
        return row, off, int(bp)

    def forward_packed(self, ids: torch.Tensor, mask: torch.Tensor | None = None, lens=None):
        """`forward` for short sentences: the B sentences share Bp <= B 128-slot rows (mec_text_fwd_packed),
        so the encoder does Bp / B of the padded batch's work. ids int32 [B,128] in the padded layout
        (a sentence's tokens first); its lengths come from `lens` (a host int array, what the tokenizer
        knows) or, without it, from `mask` (int32 [B,128], which must be a prefix mask: ones, then zeros;
        one device-to-host copy). Outputs as `forward`, in sample order; to the precision's rounding the
        values `forward(ids, prefix mask)` gives. `packed_rows` holds the plan's Bp afterwards. The GEMM
        shapes follow Bp, so a new Bp autotunes its own tiles."""
        if ids.dim() != 2 or ids.shape[1] != 128:
            raise ValueError('ids: expected [B, 128] (padding=max_length, Config.MAX_TEXT_LENGTH)')
        B = int(ids.shape[0])
        _check_tensor('ids', ids, torch.int32, (B, 128), self.device)
        if mask is not None:
            _check_tensor('mask', mask, torch.int32, (B, 128), self.device)
        if lens is None:
            if mask is None:
                raise ValueError('forward_packed: pass lens (host lengths) or mask')
            ar = torch.arange(128, device=self.device, dtype=torch.int32)
            n = mask.sum(1, dtype=torch.int32)
            prefix = (mask == (ar[None, :] < n[:, None]).to(torch.int32)).all(1)
            host = torch.stack([n, prefix.to(torch.int32)]).cpu().numpy()  # the one device-to-host copy
            if not host[1].all():
                raise ValueError('mask: forward_packed needs a prefix mask (ones, then zeros) in every row')
            lens = host[0]
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        if lens.shape != (B,):
            raise ValueError(f'lens: shape {lens.shape}, expected ({B},)')
        row, off, bp = self.pack_plan(lens)
        self.packed_rows = bp
        cls, logits, probs = self._empty(B, 768), self._empty(B, 7), self._empty(B, 7)
        if B == 0:
            return cls, logits, probs
        plan = torch.from_numpy(np.stack([row, off, lens])).to(self.device)  # one upload: row | off | len
        with self._lock:
            _lib.check(self.lib.mec_text_fwd_packed(self.handle, _ptr(ids), _ptr(plan[0]), _ptr(plan[1]),
                                                    _ptr(plan[2]), B, bp, _ptr(cls), _ptr(logits), _ptr(probs),
                                                    _stream(self.device)), 'mec_text_fwd_packed')
        plan.record_stream(torch.cuda.current_stream(self.device))
        return cls, logits, probs


class LstmTextEncoder(HipModel):
    """The reference's BiLSTM text model (model_training/train_lstm_text_model.py:96-120) on the HIP
    recurrent kernels (csrc/text_lstm.hip). fp32 at every `precision` setting, like speech and fusion."""
    kind = 'text_lstm'

    VOCAB = synthetic.LSTM_VOCAB

    def forward(self, ids: torch.Tensor, check_ids: bool = False):
        """ids int32 [B,128], post-padded with 0 -> (feat [B,64], logits [B,7], probs [B,7]).

        check_ids: raise ValueError for ids outside [0, 10000) (one device min/max reduction and a
        host sync; the batched hot path skips it, and the kernel then clamps out-of-range ids)."""
        if not isinstance(ids, torch.Tensor):
            raise TypeError(f'ids: expected a torch.Tensor, got {type(ids).__name__}')
        if ids.dim() != 2:
            raise ValueError('ids: expected [B, L]')
        B, L = ids.shape
        if L != 128:
            raise ValueError('ids: L must be 128 (pad_sequences maxlen, Config.MAX_TEXT_LENGTH)')
        _check_tensor('ids', ids, torch.int32, (B, L), self.device)
        if check_ids and B:
            lo, hi = (int(v) for v in torch.aminmax(ids))
            if lo < 0 or hi >= self.VOCAB:
                raise ValueError(f'ids: token id out of range [0, {self.VOCAB}): min {lo}, max {hi}')
        feat, logits, probs = self._empty(B, 64), self._empty(B, 7), self._empty(B, 7)
        with self._lock:
            _lib.check(self.lib.mec_text_lstm_fwd(self.handle, _ptr(ids), B, L, _ptr(feat), _ptr(logits), _ptr(probs),
                                                  _stream(self.device)), 'mec_text_lstm_fwd')
        return feat, logits, probs



class GpuTokenizer:
    """Tokenization on the GPU (mec_tok_*; csrc/tokenizer.hip): strings in, ids / mask / len on the device.

    from_keras(word_index_obj) restates KerasWordIndex.padded, from_bert(tokenizer) the BERT tokenizer
    call of inference/text_inference.py (add_special_tokens, max_length, padding='max_length',
    truncation); both give exactly the host tokenizer's integers. A text the kernel's byte-level
    specification does not cover (mec.tokenize: WORDPIECE, a text that is not 7-bit or holds a special-token
    literal; either kind, a text without a UTF-8 encoding) is tokenized by `host_rows` and its row written
    into the device result at its index, so the output order is the input order. from_bert(unicode=True)
    takes the WORDPIECE_UTF8 kind instead: any text stays on the GPU but one that holds a special-token
    literal or a code point outside the covered set (mec.tokenize.wordpiece_cpmap)."""

    def __init__(self, table: _tok.Table, host_rows, on_host=None, prepare=None, device=None, max_length: int = 128,
                 cpmap=None):
        self.lib = _lib.load()
        self.device = require_gpu(device)
        self.table, self.L, self.cpmap = table, int(max_length), cpmap
        self._host_rows, self._on_host, self._prepare = host_rows, on_host, prepare
        self.host_rows = 0  # rows the host tokenized in the last encode
        desc, keep = table.desc()
        h = ctypes.c_void_p()
        torch.cuda.set_device(self.device)
        self.handle = None
        if cpmap is None:
            _lib.check(self.lib.mec_tok_create(ctypes.byref(desc), self.device.index, ctypes.byref(h)), 'mec_tok_create')
        else:
            cp, keep_cp = cpmap.struct()
            _lib.check(self.lib.mec_tok_create_utf8(ctypes.byref(desc), ctypes.byref(cp), self.device.index,
                                                    ctypes.byref(h)), 'mec_tok_create_utf8')
            del keep_cp
        del keep
        self.handle = h

    @classmethod
    def from_keras(cls, wi, device=None, max_length: int = 128):
        """wi: a fitted word index (inference.text_lstm_inference.KerasWordIndex). ValueError when its
        split / filters are not single ASCII characters."""
        def host_rows(texts):
            seqs = [wi.sequence(t)[:max_length] for t in texts]
            ids = np.zeros((len(texts), max_length), np.int32)
            for r, s in enumerate(seqs):
                ids[r, :len(s)] = s
            n = np.array([len(s) for s in seqs], np.int32)
            return ids, (np.arange(max_length)[None, :] < n[:, None]).astype(np.int32), n
        return cls(_tok.keras_table(wi), host_rows, None, (str.lower if wi.lower else None), device, max_length)

    @classmethod
    def from_bert(cls, tokenizer, device=None, max_length: int = 128, unicode: bool = False):
        """tokenizer: a transformers BertTokenizer / BertTokenizerFast. ValueError when it has added tokens
        beyond its special tokens or strip_accents contradicts do_lower_case. unicode=True: non-ASCII text
        is tokenized on the GPU too (MEC_TOK_WORDPIECE_UTF8); ValueError unless the tokenizer lower-cases and
        strips accents."""
        def host_rows(texts):
            enc = tokenizer(list(texts), add_special_tokens=True, max_length=max_length, padding='max_length',
                            truncation=True, return_tensors='np')
            mask = enc['attention_mask'].astype(np.int32)
            return enc['input_ids'].astype(np.int32), mask, mask.sum(1).astype(np.int32)
        if unicode:
            cpmap = _tok.wordpiece_cpmap(tokenizer)
            return cls(_tok.wordpiece_table_utf8(tokenizer), host_rows,
                       _tok.wordpiece_on_host_utf8(tokenizer.all_special_tokens, cpmap), None, device, max_length, cpmap)
        return cls(_tok.wordpiece_table(tokenizer), host_rows, _tok.wordpiece_on_host(tokenizer.all_special_tokens),
                   None, device, max_length)

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.mec_tok_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode(self, texts):
        """texts: a list of str -> (ids int32 [B,L], mask int32 [B,L], len int32 [B]) on the device,
        asynchronous on the current stream: one upload each for the bytes and the offsets, one kernel, and,
        only when rows were routed to the host, one upload of those rows."""
        texts = list(texts)
        if self._prepare is not None:
            texts = [self._prepare(t) for t in texts]
        B, L = len(texts), self.L
        blob, off, host = _tok.pack_texts(texts, self._on_host)
        self.host_rows = len(host)
        ids = torch.empty((B, L), dtype=torch.int32, device=self.device)
        mask, n = torch.empty_like(ids), torch.empty((B,), dtype=torch.int32, device=self.device)
        if B == 0:
            return ids, mask, n
        text_d, off_d = to_device(blob, self.device), to_device(off, self.device)
        _lib.check(self.lib.mec_tok_encode(self.handle, _ptr(text_d), _ptr(off_d), B, L, _ptr(ids), _ptr(mask), _ptr(n),
                                           _stream(self.device)), 'mec_tok_encode')
        if host:
            h_ids, h_mask, h_n = self._host_rows([texts[i] for i in host])
            rows = torch.from_numpy(np.concatenate([h_ids, h_mask, h_n[:, None]], 1).astype(np.int32)).to(self.device)
            at = torch.tensor(host, dtype=torch.int64, device=self.device)
            ids.index_copy_(0, at, rows[:, :L])
            mask.index_copy_(0, at, rows[:, L:2 * L])
            n.index_copy_(0, at, rows[:, 2 * L])
        return ids, mask, n


class ImageEncoder(HipModel):
    kind = 'image'

    def forward(self, gray: torch.Tensor):
        """gray u8 [B,48,48] -> (feat [B,512], logits [B,7], probs [B,7])."""
        B = gray.shape[0] if gray.dim() == 3 else -1
        _check_tensor('gray', gray, torch.uint8, (B, 48, 48), self.device)
        feat, logits, probs = self._empty(B, 512), self._empty(B, 7), self._empty(B, 7)
        with self._lock:
            _lib.check(self.lib.mec_image_fwd(self.handle, _ptr(gray), B, _ptr(feat), _ptr(logits), _ptr(probs),
                                              _stream(self.device)), 'mec_image_fwd')
        return feat, logits, probs

    def forward_u8(self, img: torch.Tensor):
        """img u8 [B,H,W,C] with (H,W,C) in {(48,48,1), (224,224,1), (224,224,3)}."""
        if img.dim() == 3:
            img = img.unsqueeze(-1)
        if img.dim() != 4 or tuple(img.shape[1:]) not in ((48, 48, 1), (224, 224, 1), (224, 224, 3)):
            raise ValueError(f'img: shape {tuple(img.shape)} not in [B,48,48,1] / [B,224,224,1] / [B,224,224,3]')
        B, H, W, C = img.shape
        _check_tensor('img', img, torch.uint8, (B, H, W, C), self.device)
        feat, logits, probs = self._empty(B, 512), self._empty(B, 7), self._empty(B, 7)
        with self._lock:
            _lib.check(self.lib.mec_image_fwd_u8(self.handle, _ptr(img), B, H, W, C, _ptr(feat), _ptr(logits),
                                                 _ptr(probs), _stream(self.device)), 'mec_image_fwd_u8')
        return feat, logits, probs

    def forward_ragged(self, arrays):
        """arrays: u8 images [H,W,C] of any sizes inside the GPU resize's domain, one C (1 or 3) for all:
        resized on the GPU as PIL resizes them (resize_ragged), then forward_u8."""
        return self.forward_u8(resize_ragged(arrays, self.device))

    def x3_names(self):
        """The activation tensors with an fp32x3 plane exponent, in x3_report's order (mec_model_x3_names)."""
        r = self.lib.mec_model_x3_names(self.handle)
        if r is None:
            _lib.check(-1, 'mec_model_x3_names')
        return r.decode().split()

    def calibrate(self, batches):
        """Set this fp32x3 handle's plane exponents from observed data instead of the BatchNorm estimate.
        batches: one u8 batch (what `forward` or `forward_u8` takes), or a list of them. They run on the
        exact-fp32 twin with its observation armed (mec_model_x3_observe): max |x| of every tensor that has
        an exponent, over all the batches. The handle is then re-created from those maxima
        (mec_create_x3_calibrated: the same 64x margin to the f16 range, now over what was seen) the way
        `x3_widen` re-creates it, and keeps them: a later `x3_widen` adds its headroom on top.
        -> {tensor name: (observed max |x|, exponent s)}. ValueError unless precision is 'fp32x3'."""
        if self.precision != 'fp32x3':
            raise ValueError(f"calibrate: an fp32x3 handle's plane exponents are calibrated; this one is {self.precision}")
        batches = [batches] if isinstance(batches, torch.Tensor) else list(batches)
        if not batches:
            raise ValueError('calibrate: no batch to observe')
        twin = self.fp32_twin()
        with torch.cuda.device(self.device):
            n = self.lib.mec_model_x3_observe(twin.handle, 1)
            if n < 0:
                _lib.check(n, 'mec_model_x3_observe')
            try:
                for x in batches:
                    twin.forward(x) if x.dim() == 3 else twin.forward_u8(x)
                seen = np.zeros(n, np.float32)
                if self.lib.mec_model_x3_observed(twin.handle, seen.ctypes.data_as(_lib.c_fp), n) != n:
                    _lib.check(-1, 'mec_model_x3_observed')  # (it synchronized the device)
            finally:
                self.lib.mec_model_x3_observe(twin.handle, 0)
        twin.check()
        names = self.x3_names()
        if not np.isfinite(seen).all():
            raise MecError('calibrate: an inf or a NaN in ' + ', '.join(k for k, v in zip(names, seen) if not np.isfinite(v)))
        self._x3_cal = seen
        self._recreate(self._copts)
        s = {ln.split()[0]: int(ln.split()[1][2:]) for ln in self.x3_report().splitlines()[1:]}
        return {k: (float(v), s[k]) for k, v in zip(names, seen)}


def resize_ragged(arrays, device=None, channels: int = 3) -> torch.Tensor:
    """A list of u8 images [H,W,C] (or [H,W]) that share one C in {1, 3} -> u8 [B,224,224,C] on the device,
    each image resized as PIL's `resize((224, 224), Image.BILINEAR)` resizes it, byte for byte
    (mec_resize_ragged_u8; csrc/resize.hip). Every image must lie in the domain mec.image.resize_on_gpu
    states (ValueError otherwise: the caller routes the others to the host). The images are packed into one
    pinned staging buffer and uploaded in one copy; the intermediate and the result are torch allocations.
    Asynchronous on the current stream. `channels` only gives an empty list its C."""
    lib = _lib.load()
    dev = require_gpu(device)
    arrs = []
    for i, a in enumerate(arrays):
        arrs.append(_image.check_image(i, a, arrs[0].shape[2] if arrs else None))
    C = arrs[0].shape[2] if arrs else int(channels)
    if C not in (1, 3):
        raise ValueError(f'C must be 1 or 3, got {C}')
    hw = np.array([a.shape[:2] for a in arrs], np.int32).reshape(-1, 2)
    offs, _, total = _image.pack_layout([a.size for a in arrs])
    with torch.cuda.device(dev):
        src = _pinned(total, zip(offs, arrs)).to(dev, non_blocking=True) if arrs else None
        return _resize_on_device(lib, src, offs, hw, C, total, dev)


def _pinned(total, pieces) -> torch.Tensor:
    """A pinned u8 staging tensor of `total` bytes holding each (offset, u8 array) of `pieces`."""
    stage = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    view = stage.numpy()
    for o, a in pieces:
        view[o:o + a.size] = a.reshape(-1)
    return stage


def _resize_on_device(lib, src, offs, hw, C, src_bytes, dev) -> torch.Tensor:
    """mec_resize_ragged_u8 on the images at `offs` (int64 [B]) of the device buffer `src`, of extents `hw`
    (int32 [B,2]) and C channels -> u8 [B,224,224,C]. Allocates the result and the horizontal pass'
    intermediate, sum(H) * 224 * C bytes; an empty batch makes no call. `dev` is the current device."""
    B = len(offs)
    out = torch.empty((B, _image.OUT, _image.OUT, C), dtype=torch.uint8, device=dev)
    if B:
        tmp_bytes = int(hw[:, 0].astype(np.int64).sum()) * _image.OUT * C
        tmp = torch.empty(tmp_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.mec_resize_ragged_u8(_ptr(src), offs.ctypes.data, hw.ctypes.data, B, C, src_bytes, _ptr(tmp),
                                            tmp_bytes, _ptr(out), _stream(dev)), 'mec_resize_ragged_u8')
    return out


def _jpeg_decode(lib, buf, src_bytes, blobs, scan_offs, dst_at, dst_offs, dst_bytes, status, dev):
    """mec_jpeg_decode_ragged on `blobs` (mec.jpeg.Blob) whose scans lie at `scan_offs` of the device buffer `buf`
    (src_bytes of it are sources): image k is written at buf + dst_at + dst_offs[k] (dst_bytes of room) and its
    status into the device int32 tensor `status`. Allocates the workspace; `dev` is the current device."""
    descs = _jpeg.desc_array([b.desc for b in blobs])
    segs = np.ascontiguousarray(np.concatenate(
        [b.segs + np.array([[int(o) - b.span[0], 0]], np.int64) for b, o in zip(blobs, scan_offs)]), np.int64)
    ws_bytes = _jpeg.workspace_bytes([b.desc for b in blobs])
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    dst_offs = np.ascontiguousarray(dst_offs, np.int64)
    _lib.check(lib.mec_jpeg_decode_ragged(_ptr(buf), src_bytes, ctypes.addressof(descs), segs.ctypes.data, len(blobs),
                                          ctypes.c_void_p(buf.data_ptr() + dst_at), dst_offs.ctypes.data, dst_bytes,
                                          _ptr(ws), ws_bytes, _ptr(status), _stream(dev)), 'mec_jpeg_decode_ragged')


def decode_jpeg_ragged(blobs, device=None):
    """A list of probed files (mec.jpeg.Blob) -> (images, status): images[k] is a device u8 tensor [H,W,C], C = 1
    (Pillow's L) or 3 (RGB), holding what `Image.open(file).load()` gives, byte for byte; status is a device int32
    tensor [B], 0 for a decoded image, else mec.jpeg.ST_* (the image's bytes are then unspecified: the caller
    decodes that file on the host). The scans are packed into one pinned buffer and uploaded in one copy; the
    images lie behind them in the same device buffer (mec_jpeg_decode_ragged; csrc/jpeg.hip). Asynchronous on the
    current stream."""
    lib = _lib.load()
    dev = require_gpu(device)
    B = len(blobs)
    status = torch.zeros(B, dtype=torch.int32, device=dev)
    if B == 0:
        return [], status
    scans = [b.scan() for b in blobs]
    offs, _, end = _image.pack_layout([a.size for a in scans])
    src_total = _image.pad16(end)
    dst_offs, _, dst_end = _image.pack_layout([b.out_bytes for b in blobs])
    room = _image.pad16(dst_end)
    with torch.cuda.device(dev):
        buf = torch.empty(src_total + room, dtype=torch.uint8, device=dev)
        buf[:src_total].copy_(_pinned(src_total, zip(offs, scans)), non_blocking=True)
        _jpeg_decode(lib, buf, src_total, blobs, offs, src_total, dst_offs, room, status, dev)
    images = [buf[src_total + int(o):src_total + int(o) + b.out_bytes].view(b.H, b.W, b.C) for b, o in zip(blobs, dst_offs)]
    return images, status


def ingest_ragged(items, device=None):
    """A list of (u8 array, fmt, palette or None) -- images in their native pixel formats, fmt one of
    mec.image.PIX_* ([H,W] or [H,W,bpp]; a PIX_P image with its palette, u8 [768]) -> (gray, groups): gray is a
    bool array [B], what the host's R == G == B test on the RGB-converted pixels gives; groups is
    [(u8 [n48,48,48,1], rows), (u8 [n1,224,224,1], rows), (u8 [n3,224,224,3], rows)], device tensors holding
    what `convert('RGB')`, the gray test, the channel selection and `resize((224, 224), Image.BILINEAR)` give on
    the host, byte for byte, and the ascending indices into `items` of each tensor's rows: gray 48 x 48 images
    as they are, every other gray image's one channel resized, every other image's RGB resized.

    The images and the distinct palettes are packed into one pinned buffer and uploaded in one copy into a device
    buffer with room behind them for the converted images. mec_image_gray_ragged_u8 tests them there and the B
    flags are read back (the one synchronisation of the call: c_out and the groups depend on them);
    mec_image_canon_ragged_u8 converts the images whose native bytes are not what their consumer reads, and one
    mec_resize_ragged_u8 call per channel count reads untouched and converted images from the same buffer. Every
    image must lie in mec.image.resize_on_gpu's domain (ValueError otherwise)."""
    gray, groups, _ = ingest_ragged_files(items, device)
    return gray, groups


def ingest_ragged_files(items, device=None):
    """`ingest_ragged` for a batch that mixes its items with undecoded JPEG files (mec.jpeg.Blob, what
    mec.jpeg.probe returns for a file of the GPU decoder's domain) -> (gray, groups, status). A file's scan goes up
    in the same single copy as the other items' pixels; mec_jpeg_decode_ragged decodes the files into room behind
    the sources, where the gray test, the conversion and the resize read them as PIX_L / PIX_RGB images like any
    other. status is an int32 array [B]: 0 for every item but a file the kernels gave up (mec.jpeg.ST_*), which is
    in no group and whose gray flag means nothing: the caller decodes it on the host. The statuses are read back
    with the gray flags, in the call's one synchronisation."""
    lib = _lib.load()
    dev = require_gpu(device)
    B = len(items)
    isblob = [isinstance(it, _jpeg.Blob) for it in items]
    arrs, pals = [], []
    for i, it in enumerate(items):
        if isblob[i]:
            if not _image.resize_on_gpu(it.H, it.W):
                raise ValueError(f'image {i}: {it.H} x {it.W} is outside the GPU resize\'s domain')
            arrs.append(it.scan())
            pals.append(None)
            continue
        a, fmt, pal = it
        arrs.append(_image.check_image(i, a, fmt=fmt, pal=pal))
        if pal is not None:
            pal = np.ascontiguousarray(pal, np.uint8).reshape(-1)
            if pal.size != _image.PAL_BYTES:
                raise ValueError(f'image {i}: the palette must hold 768 bytes (256 RGB entries, zero-padded)')
            pal = pal.tobytes()
        pals.append(pal)
    if B == 0:
        return (np.zeros(0, bool), [(torch.empty((0,) + s, dtype=torch.uint8, device=dev), []) for s in _image.MODEL_SHAPES],
                np.zeros(0, np.int32))
    fmts = np.array([it.fmt if b else it[1] for it, b in zip(items, isblob)], np.int32)
    hw = np.array([(it.H, it.W) if b else a.shape[:2] for it, b, a in zip(items, isblob, arrs)], np.int32).reshape(B, 2)
    up_offs, pal_at, end = _image.pack_layout([a.size for a in arrs], [p for p in pals if p is not None])
    pal_off = np.array([-1 if p is None else pal_at[p] for p in pals], np.int64)
    src_total = _image.pad16(end)
    # the decoded files follow the sources; from there on they are images like the others
    blob_at = np.array([i for i in range(B) if isblob[i]], np.int64)
    blobs = [items[i] for i in blob_at]
    dec_offs, _, dec_end = _image.pack_layout([b.out_bytes for b in blobs])
    dec_total = src_total + _image.pad16(dec_end)
    offs = up_offs.copy()
    offs[blob_at] = src_total + dec_offs
    cap = sum(_image.canon_room(f, H, W) for f, (H, W) in zip(fmts, hw.tolist()))  # the most the converted images take
    total = dec_total + cap
    stage = _pinned(src_total, list(zip(up_offs, arrs)) + [(o, np.frombuffer(p, np.uint8)) for p, o in pal_at.items()])
    with torch.cuda.device(dev):
        stream = _stream(dev)
        buf = torch.empty(total, dtype=torch.uint8, device=dev)
        buf[:src_total].copy_(stage, non_blocking=True)
        flags_d = torch.empty(B + len(blobs), dtype=torch.int32, device=dev)  # the gray flags, then the files' statuses
        if blobs:
            _jpeg_decode(lib, buf, src_total, blobs, up_offs[blob_at], src_total, dec_offs, dec_total - src_total,
                         flags_d[B:], dev)
        _lib.check(lib.mec_image_gray_ragged_u8(_ptr(buf), offs.ctypes.data, hw.ctypes.data, fmts.ctypes.data,
                                                pal_off.ctypes.data, B, dec_total, _ptr(flags_d), stream),
                   'mec_image_gray_ragged_u8')
        flags_h = torch.empty(B + len(blobs), dtype=torch.int32, pin_memory=True)
        flags_h.copy_(flags_d, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()
        gray = flags_h.numpy()[:B].astype(bool)
        status = np.zeros(B, np.int32)
        status[blob_at] = flags_h.numpy()[B:]
        ok = np.flatnonzero(status == 0)  # a file the kernels gave up is no image from here on
        offs, hw, fmts, pal_off = (np.ascontiguousarray(a[ok]) for a in (offs, hw, fmts, pal_off))
        face, chan, c_out, dst_offs, read_at = _image.canon_plan(gray[ok], hw, fmts, offs, dec_total)
        if c_out.any():
            _lib.check(lib.mec_image_canon_ragged_u8(
                _ptr(buf), offs.ctypes.data, hw.ctypes.data, fmts.ctypes.data, pal_off.ctypes.data,
                c_out.ctypes.data, dst_offs.ctypes.data, len(ok), dec_total, ctypes.c_void_p(buf.data_ptr() + dec_total),
                cap, stream), 'mec_image_canon_ragged_u8')
        n48 = int(face.sum())
        groups = [(buf[dec_total:dec_total + n48 * 2304].view(n48, 48, 48, 1), [int(i) for i in ok[np.flatnonzero(face)]])]
        for C in (1, 3):
            rows = np.flatnonzero(~face & (chan == C))
            out = _resize_on_device(lib, buf, np.ascontiguousarray(read_at[rows]), np.ascontiguousarray(hw[rows]), C,
                                    total, dev)
            groups.append((out, [int(i) for i in ok[rows]]))
    return gray, groups, status


def jpeg_prof(on: bool):
    """Switch the hipEvent timing of the JPEG decode's three kernels on or off (process-wide)."""
    _lib.check(_lib.load().mec_jpeg_prof_enable(int(bool(on))), 'mec_jpeg_prof_enable')


def jpeg_prof_read():
    """(entropy ms, IDCT ms, upsample / colour ms, calls) since the last read or enable; synchronizes on the events."""
    e, i, c, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _lib.check(_lib.load().mec_jpeg_prof_read(ctypes.byref(e), ctypes.byref(i), ctypes.byref(c), ctypes.byref(n)),
               'mec_jpeg_prof_read')
    return e.value, i.value, c.value, n.value


def canon_prof(on: bool):
    """Switch the hipEvent timing of the gray and conversion kernels on or off (process-wide)."""
    _lib.check(_lib.load().mec_image_canon_prof_enable(int(bool(on))), 'mec_image_canon_prof_enable')


def canon_prof_read():
    """(gray ms, gray launches, conversion ms, conversion launches) since the last read or enable."""
    g, c, ng, nc = ctypes.c_double(), ctypes.c_double(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().mec_image_canon_prof_read(ctypes.byref(g), ctypes.byref(ng), ctypes.byref(c),
                                                     ctypes.byref(nc)), 'mec_image_canon_prof_read')
    return g.value, ng.value, c.value, nc.value


def resize_prof(on: bool):
    """Switch the hipEvent timing of the ragged resize's two kernels on or off (process-wide)."""
    _lib.check(_lib.load().mec_resize_prof_enable(int(bool(on))), 'mec_resize_prof_enable')


def resize_prof_read():
    """(horizontal ms, vertical ms, calls) since the last read or enable; synchronizes on the events."""
    h, v, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _lib.check(_lib.load().mec_resize_prof_read(ctypes.byref(h), ctypes.byref(v), ctypes.byref(n)),
               'mec_resize_prof_read')
    return h.value, v.value, n.value


class MobileNetImageEncoder(ImageEncoder):
    """The same image entry points on the MobileNetV2 backbone (csrc/mobilenet.hip)."""
    kind = 'image_mbv2'


IMAGE_BACKBONES = {'resnet50': ImageEncoder, 'mobilenet_v2': MobileNetImageEncoder}

AUDIO_KIND = 5  # include/mec.h MEC_AUDIO
N_FFT, HOP, N_MELS = 2048, 512, 128  # librosa defaults the reference never overrides


class AudioFeaturizer(HipModel):
    """preprocess_audio's 56-d speech features (preprocessing/audio_preprocessing.py:22-46:
    mean MFCC-40 | mean chroma-12 | mean zcr, centroid, rolloff, rms) computed on the GPU
    (csrc/audio.hip) for a batch of fixed-length waveforms (load_audio's pad/trim applied)."""
    kind = 'audio'

    def __init__(self, sample_rate: int = 22050, n_mfcc: int = 40, device=None):
        self.lib = _lib.load()
        self.device = require_gpu(device)
        self.precision = 'fp32'
        self.sample_rate, self.n_mfcc = int(sample_rate), int(n_mfcc)
        self._knobs, self._twin, self._copts, self.x3_reruns = [], None, {}, 0
        self.n_features = self.n_mfcc + 16
        blob = np.array([sample_rate, N_FFT, HOP, N_MELS, n_mfcc], np.float32)
        h = ctypes.c_void_p()
        torch.cuda.set_device(self.device)
        _lib.check(self.lib.mec_create_ex(AUDIO_KIND, blob.ctypes.data_as(_lib.c_fp), blob.size, self.device.index,
                                          _lib.PRECISIONS['fp32'], ctypes.byref(h)), 'mec_create(audio)')
        self.handle = h
        self._lock = threading.Lock()

    def forward(self, wave: torch.Tensor, return_tuning: bool = False):
        """wave f32 [B, n] -> features f32 [B, n_mfcc + 16] (and the chroma tuning [B])."""
        if wave.dim() != 2:
            raise ValueError('wave: expected [B, n_samples]')
        B, n = wave.shape
        _check_tensor('wave', wave, torch.float32, (B, n), self.device)
        feat = self._empty(B, self.n_features)
        tun = self._empty(B) if return_tuning else None
        with self._lock:
            _lib.check(self.lib.mec_audio_fwd(self.handle, _ptr(wave), B, n, _ptr(feat), _ptr(tun),
                                              _stream(self.device)), 'mec_audio_fwd')
        return (feat, tun) if return_tuning else feat


class AudioLoader:
    """load_audio on the GPU for PCM clips (mec_audio_load_ragged; csrc/audio_load.hip): a ragged batch of
    (bytes, fmt, channels, rate, frames) clips, as mec.wav.read_clip gives them, is packed into one pinned
    staging buffer, uploaded in one copy, and decoded, mixed to mono, resampled to the featurizer's rate and
    padded or trimmed to n_out = 3 s on the device -> f32 [B, n_out], what AudioFeaturizer.forward takes.
    It shares the featurizer's handle (the tap tables are cached there). Asynchronous on the current stream."""

    def __init__(self, featurizer: 'AudioFeaturizer', n_out: int | None = None):
        self.audio = featurizer
        self.device = featurizer.device
        self.sample_rate = featurizer.sample_rate
        self.n_out = int(n_out) if n_out is not None else 3 * featurizer.sample_rate

    def load(self, clips) -> torch.Tensor:
        clips = list(clips)
        B, dev = len(clips), self.device
        views = [np.frombuffer(c[0], np.uint8) for c in clips]
        desc = np.array([c[1:5] for c in clips], np.int32).reshape(-1, 4)
        offs, _, total = _image.pack_layout([v.size for v in views])
        with torch.cuda.device(dev):
            wave = torch.empty((B, self.n_out), dtype=torch.float32, device=dev)
            if B:
                src = _pinned(total, zip(offs, views)).to(dev, non_blocking=True) if total else None
                with self.audio._lock:
                    _lib.check(self.audio.lib.mec_audio_load_ragged(
                        self.audio.handle, _ptr(src), offs.ctypes.data, desc.ctypes.data, B, total, _ptr(wave),
                        self.n_out, _stream(dev)), 'mec_audio_load_ragged')
        return wave

    def read_one(self, path):
        """mec.wav.read_clip for this loader's rate and length: the clip, or None for a file it declines."""
        return _wav.read_clip(path, self.sample_rate, self.n_out / self.sample_rate)

    def read(self, paths):
        """-> (clips, at, declined): the clips of the files mec.wav.read_clip takes, their positions in
        `paths`, and the positions of the files it declines (for the host loader)."""
        clips, at, declined = [], [], []
        for i, p in enumerate(paths):
            c = self.read_one(p)
            (declined if c is None else at).append(i)
            if c is not None:
                clips.append(c)
        return clips, at, declined


def audio_load_prof(on: bool):
    """hipEvent timing of the audio front end's kernel (mec_audio_load_prof_enable), process-wide."""
    _lib.check(_lib.load().mec_audio_load_prof_enable(1 if on else 0), 'mec_audio_load_prof_enable')


def audio_load_prof_read():
    """(kernel ms, calls) since the last read or enable; synchronizes on the events."""
    ms, n = ctypes.c_double(), ctypes.c_int()
    _lib.check(_lib.load().mec_audio_load_prof_read(ctypes.byref(ms), ctypes.byref(n)), 'mec_audio_load_prof_read')
    return ms.value, n.value


class FusionHead(HipModel):
    kind = 'fusion'

    def forward(self, s_feat, t_feat, i_feat, s_pred, t_pred, i_pred):
        """-> (logits [B,7], probs [B,7], attn_w [B,3], dec_w [B,3])."""
        B = s_feat.shape[0]
        for n, t, d in (('s_feat', s_feat, 64), ('t_feat', t_feat, 768), ('i_feat', i_feat, 512),
                        ('s_pred', s_pred, 7), ('t_pred', t_pred, 7), ('i_pred', i_pred, 7)):
            _check_tensor(n, t, torch.float32, (B, d), self.device)
        logits, probs, aw, dw = self._empty(B, 7), self._empty(B, 7), self._empty(B, 3), self._empty(B, 3)
        with self._lock:
            _lib.check(self.lib.mec_fusion_fwd(self.handle, _ptr(s_feat), _ptr(t_feat), _ptr(i_feat), _ptr(s_pred),
                                               _ptr(t_pred), _ptr(i_pred), B, _ptr(logits), _ptr(probs), _ptr(aw),
                                               _ptr(dw), _stream(self.device)), 'mec_fusion_fwd')
        return logits, probs, aw, dw

    def forward_mixed(self, plan, speech, text, image):
        """The fusion step of a mixed-modality batch (mec_fusion_fwd_mixed). plan: a `fusion_mixed_plan`
        made with have_model=True; speech / text / image: a `(feat, probs)` pair of compact tensors
        ([ns,64] / [nt,768] / [ni,512] and [n,7], the rows that have the modality in sample order), or None
        when the plan's count is 0. -> (fused f64 [B,7], logits [B,7], attn_w [B,3], dec_w [B,3]): every
        sample routed as predict_multimodal routes a request; zeros in the last three off the attention
        route."""
        if not plan.have_model:
            raise ValueError('forward_mixed: the plan was made with have_model=False (engine.fuse_mixed takes it)')
        with self._lock:
            return _fusion_mixed(self.lib, self.handle, plan, (speech, text, image), self.device)


class FusionMixedPlan:
    """A mixed batch's routing (mec_fusion_mixed_plan): host `present` (bitmask uint8 [B]), `route`
    (ROUTE_* int32 [B]), `s_idx` / `t_idx` / `i_idx` / `att` (int32 [B]), `counts` = (ns, nt, ni), `n_att`,
    `have_model`; `dev` holds s_idx | t_idx | i_idx | att as one int32 [4,B] device tensor."""

    def __init__(self, present, have_model, route, idx, att, counts, n_att, dev):
        self.present, self.have_model, self.route = present, bool(have_model), route
        self.s_idx, self.t_idx, self.i_idx = idx
        self.att, self.counts, self.n_att, self.dev = att, tuple(int(c) for c in counts), int(n_att), dev
        self.B = int(present.size)

    def rows(self, route):
        """The samples on `route` (a _lib.ROUTE_* value), ascending."""
        return np.flatnonzero(self.route == route)


def fusion_mixed_plan(present, have_model: bool = True, device=None) -> FusionMixedPlan:
    """present: a host bool / uint8 array [B,3] (speech, text, image) or a bitmask [B] (an or of
    _lib.MOD_SPEECH / MOD_TEXT / MOD_IMAGE) -> the plan, its index arrays uploaded once to `device`.
    have_model=False: no attention model, samples with all three modalities take the average."""
    lib = _lib.load()
    dev = require_gpu(device)
    p = np.asarray(present)
    if p.ndim == 2 and p.shape[1] == 3:
        p = (p != 0).astype(np.uint8) @ np.array([1, 2, 4], np.uint8)
    elif p.ndim != 1:
        raise ValueError(f'present: shape {p.shape}, expected [B,3] flags or a [B] bitmask')
    elif p.size and (p.min() < 0 or p.max() > 7):
        raise ValueError('present: a bitmask entry outside [0, 7]')
    p = np.ascontiguousarray(p, dtype=np.uint8)
    B = int(p.size)
    arr = np.full((5, B), -1, np.int32)  # s_idx | t_idx | i_idx | att | route
    counts = np.zeros(3, np.int32)
    ip = ctypes.POINTER(ctypes.c_int32)
    a = [arr[k].ctypes.data_as(ip) for k in range(5)]
    n_att = lib.mec_fusion_mixed_plan(p.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), B, int(bool(have_model)),
                                      a[0], a[1], a[2], a[4], a[3], counts.ctypes.data_as(ip))
    if n_att < 0:
        _lib.check(n_att, 'mec_fusion_mixed_plan')
    return FusionMixedPlan(p, have_model, arr[4], (arr[0], arr[1], arr[2]), arr[3], counts, n_att,
                           torch.from_numpy(arr[:4].copy()).to(dev))


def _fusion_mixed(lib, handle, plan, pairs, dev):
    if not isinstance(plan, FusionMixedPlan):
        raise TypeError(f'plan: expected a FusionMixedPlan (engine.fusion_mixed_plan), got {type(plan).__name__}')
    B = plan.B
    _check_tensor('plan.dev', plan.dev, torch.int32, (4, B), dev)
    ptrs = []
    for name, d, n, pair in zip(('speech', 'text', 'image'), (64, 768, 512), plan.counts, pairs):
        if pair is None:
            if n:
                raise ValueError(f'{name}: None, but the plan has {n} samples with it')
            ptrs.append((None, None))
            continue
        feat, pred = pair if handle is not None else (None, pair)
        if feat is not None:
            _check_tensor(f'{name} feat', feat, torch.float32, (n, d), dev)
        _check_tensor(f'{name} probs', pred, torch.float32, (n, 7), dev)
        ptrs.append((feat if n else None, pred if n else None))
    fused = torch.empty((B, 7), dtype=torch.float64, device=dev)
    logits, aw, dw = (torch.empty((B, k), dtype=torch.float32, device=dev) for k in (7, 3, 3))
    if B == 0:
        return fused, logits, aw, dw
    (sf, sp), (tf, tp), (imf, ip) = ptrs
    ns, nt, ni = plan.counts
    args = _lib.FusionMixedArgs(s_feat=_ptr(sf), t_feat=_ptr(tf), i_feat=_ptr(imf), s_pred=_ptr(sp), t_pred=_ptr(tp),
                                i_pred=_ptr(ip), ns=ns, nt=nt, ni=ni, s_idx=_ptr(plan.dev[0]), t_idx=_ptr(plan.dev[1]),
                                i_idx=_ptr(plan.dev[2]), att=_ptr(plan.dev[3]), n_att=plan.n_att, B=B,
                                fused=_ptr(fused), logits=_ptr(logits), attn_w=_ptr(aw), dec_w=_ptr(dw))
    _lib.check(lib.mec_fusion_fwd_mixed(handle, ctypes.byref(args), _stream(dev)), 'mec_fusion_fwd_mixed')
    plan.dev.record_stream(torch.cuda.current_stream(dev))
    return fused, logits, aw, dw


def fuse_mixed(plan, s_pred=None, t_pred=None, i_pred=None):
    """`FusionHead.forward_mixed` without an attention model (the null handle; a plan made with
    have_model=False): compact probs [ns,7] / [nt,7] / [ni,7] (None when the count is 0) ->
    (fused f64 [B,7], logits, attn_w, dec_w), the last three all zeros. Samples with two or three
    modalities take the float64 average."""
    if isinstance(plan, FusionMixedPlan) and plan.have_model:
        raise ValueError('fuse_mixed: the plan was made with have_model=True (FusionHead.forward_mixed takes it)')
    return _fusion_mixed(_lib.load(), None, plan, (s_pred, t_pred, i_pred), plan.dev.device)


def fuse_weighted(s=None, t=None, i=None, device=None) -> torch.Tensor:
    """Weighted-average fallback on the GPU (float64) -> [B,7] f64; None = missing modality."""
    present = [x for x in (s, t, i) if x is not None]
    lib = _lib.load()
    dev = present[0].device if present else require_gpu(device)
    B = present[0].shape[0] if present else 1
    for n, x in (('s', s), ('t', t), ('i', i)):
        if x is not None:
            _check_tensor(n, x, torch.float32, (B, 7), dev)
    out = torch.empty((B, 7), dtype=torch.float64, device=dev)
    _lib.check(lib.mec_fuse_weighted(_ptr(s), _ptr(t), _ptr(i), B, _ptr(out), _stream(dev)), 'mec_fuse_weighted')
    return out


def fuse_weighted_f64(s=None, t=None, i=None, device=None) -> torch.Tensor:
    """Same as fuse_weighted with float64 [B,7] inputs (per-request Python floats)."""
    present = [x for x in (s, t, i) if x is not None]
    lib = _lib.load()
    dev = present[0].device if present else require_gpu(device)
    B = present[0].shape[0] if present else 1
    for n, x in (('s', s), ('t', t), ('i', i)):
        if x is not None:
            _check_tensor(n, x, torch.float64, (B, 7), dev)
    out = torch.empty((B, 7), dtype=torch.float64, device=dev)
    _lib.check(lib.mec_fuse_weighted_f64(_ptr(s), _ptr(t), _ptr(i), B, _ptr(out), _stream(dev)),
               'mec_fuse_weighted_f64')
    return out


# Packed per-sample result row gathered across ranks: 3x7 modality probs,
# 7 fused probs, 3 attention weights, 3 decision weights = 34 floats.
ROW = 34


class FusedPipeline:
    """The whole tri-modal path: speech + text + image encoders, then the fusion model.

    BERT runs on a high-priority stream (text_priority; else the caller's stream); speech and
    the image backbone run concurrently on a second HIP stream at normal priority, so BERT's
    workgroups are dispatched first and the image kernels fill the CUs that BERT's GEMM tails
    and its LayerNorm/attention kernels leave idle (+1.5% over equal priorities). The first
    call runs everything serially so each GEMM shape is autotuned in isolation.

    pipelined=True (the default with concurrent=True): the fusion model (and the caller's
    `epilogue`, e.g. packing and the all-gather) runs on a third stream that waits for both
    encoder streams, and the caller's stream does NOT wait for it. Consecutive batches
    therefore overlap: batch i's fusion (a latency-bound kernel of ~128 workgroups) runs
    under batch i+1's BERT instead of idling the GPU between them. Every batch's work is still
    done; outputs are ready once `wait()` (or a device synchronize) returns.
    """

    def __init__(self, seed: int = 1234, device=None, weights=None, concurrent: bool = True,
                 image_backbone: str = 'resnet50', pipelined: bool = True, text_priority: bool = True,
                 image_priority: bool = False, precision: str = 'f16'):
        weights = weights or {}
        self.precision = precision
        self.speech = SpeechEncoder(weights.get('speech'), seed, device)
        self.text = TextEncoder(weights.get('text'), seed, device, precision)
        self.image = IMAGE_BACKBONES[image_backbone](weights.get('image'), seed, device, precision)
        self.fusion = FusionHead(weights.get('fusion'), seed, device)
        self.device = self.speech.device
        self.concurrent = concurrent
        self.pipelined = concurrent and pipelined
        # image_priority (A/B): the speech + image stream at high priority instead, BERT on its
        # own normal-priority stream
        self._side = (torch.cuda.Stream(device=self.device, priority=-1 if image_priority else 0)
                      if concurrent else None)
        self._tail = torch.cuda.Stream(device=self.device) if self.pipelined else None
        # text_priority: BERT on its own high-priority stream, so its workgroups are dispatched
        # ahead of the image stream's and the image kernels fill the CUs BERT leaves idle
        self._text = (torch.cuda.Stream(device=self.device, priority=0 if image_priority else -1)
                      if (concurrent and (text_priority or image_priority)) else None)
        self._tuned = set()  # batch sizes B, or (B, packed rows Bp), whose GEMM shapes were autotuned (serially)
        self._tuned_mixed = set()  # the same for forward_mixed: (text key, ni), the text key nt or (nt, Bp)
        self._last, self._since_check = None, 0
        if concurrent and precision == 'f16':
            # BERT FFN2 (M = 128 B, N = 768, K = 3072) on the 256 x 256 ping-pong tile beside the
            # image stream: BERT alone runs it fastest on 128 x 128 (the autotuner's pick, text
            # 7.90 vs 8.02 ms at B = 256), but in the concurrent step the 4x fewer, larger tiles
            # win: 11.10 vs 11.37 ms per step (interleaved A/B, tools/gpu_ab_tiles.sh,
            # profiles/r02_ab_tiles_fused.txt). Same k order on both tiles: same bits.
            self.text.set_option('gemm_bn_tag', TAG_BERT_FFN2 * 100000 + 40256)
        if concurrent and precision == 'fp32x3':
            # the same for the fp32x3 path: FFN2 on the 256 x 256 K-interleaved split tile (384 tiles,
            # 1.5 rounds of 256 CUs: the image stream fills the half-empty round) instead of the
            # autotuner's 128 x 128 / 256 x 128 pick: 26.62 vs 27.49 ms per step (interleaved A/B,
            # tools/gpu_ab_x3tags.sh, profiles/r03_ab_x3tag_ffn2.txt). Every interleaved tile gives
            # the same bits.
            self.text.set_option('gemm_x3_tag', TAG_BERT_FFN2 * 100000 + 70256)
            # the O-projection (N = 768) the same way, since the fused QKV kernels share CUs two at a
            # time: 25.00 vs 25.21 ms per step (11 interleaved rounds, profiles/r04_ab_x3tag_oproj2.txt;
            # within 0.3 % in round 3, before that change)
            self.text.set_option('gemm_x3_tag', TAG_BERT_OPROJ * 100000 + 70256)
            # QKV (N = 2304: 1152 tiles, 4.5 rounds) on the same tile, which the autotuner picks alone
            # too but not on every run: 25.45 vs 25.58 ms per step autotuned, 256 x 128 / 128 x 128
            # 25.95 / 25.86 (profiles/r03_ab_x3tag_qkv.txt)
            self.text.set_option('gemm_x3_tag', TAG_BERT_QKV * 100000 + 70256)

    def forward(self, x_speech, ids, mask, gray, epilogue=None, text_lens=None):
        """One batch through the path -> dict of per-modality and fusion outputs (and, with
        `epilogue`, ``(outputs, epilogue(outputs))``, the callable run on the fusion's stream).

        text_lens (a host int array of the B sentence lengths, each in [1,128]; None = the padded path):
        the text leg runs packed (TextEncoder.forward_packed) on the text stream. The plan's Bp sets
        BERT's GEMM shapes (M = 128 Bp), so the serial first-batch autotune rule applies per (B, Bp): the
        first batch of a Bp not seen with this B runs serially."""
        B = int(ids.shape[0])
        if text_lens is None:
            text_fwd, key = (lambda: self.text.forward(ids, mask)), B
        else:
            text_lens = np.ascontiguousarray(text_lens, dtype=np.int32)
            key = (B, self.text.pack_plan(text_lens)[2])
            text_fwd = lambda: self.text.forward_packed(ids, mask, text_lens)  # noqa: E731
        (sf, sl, sp), (tf, tl, tp), (imf, il, ip), fstream = self._encoders(
            key, self._tuned, lambda: self.speech.forward(x_speech), text_fwd, lambda: self.image.forward(gray),
            (x_speech, gray), (ids, mask))
        with torch.cuda.stream(fstream):
            fl, fp, aw, dw = self.fusion.forward(sf, tf, imf, sp, tp, ip)
            out = {'speech': (sf, sl, sp), 'text': (tf, tl, tp), 'image': (imf, il, ip),
                   'fusion': (fl, fp, aw, dw)}
            extra = epilogue(out) if epilogue is not None else None
        self._record(out, ids, mask, gray, text_lens)
        return out if epilogue is None else (out, extra)

    def _record(self, out, ids, mask, gray, text_lens):
        self._last = {'text': (ids, mask), 'image': (gray,), 'out': out}  # check() repairs this batch
        if text_lens is not None:
            self._last.update(text=(ids, mask, text_lens), text_method='forward_packed')
        self._since_check += 1

    def _encoders(self, key, tuned, speech_fwd, text_fwd, image_fwd, side_in, text_in):
        """The three encoder legs of one batch on their streams -> (speech, text, image output tuples, the
        stream the fusion runs on). `key` not in `tuned` (or concurrent=False): everything serially on the
        caller's stream. side_in / text_in: the input tensors the side / text stream reads."""
        main = torch.cuda.current_stream(self.device)
        if not self.concurrent or key not in tuned:
            # a batch size not seen yet runs serially on one stream, so each new GEMM shape is
            # autotuned alone (not against the other encoder's kernels)
            for st in (self._side, self._text, self._tail):  # nothing else in flight while tuning
                if st is not None:
                    main.wait_stream(st)
            sf, sl, sp = speech_fwd()
            tf, tl, tp = text_fwd()
            imf, il, ip = image_fwd()
            tuned.add(key)
            fstream = main
        else:
            side = self._side
            side.wait_stream(main)  # inputs were produced on the main stream
            with torch.cuda.stream(side):
                sf, sl, sp = speech_fwd()
                imf, il, ip = image_fwd()
            if self._text is not None:
                tstream = self._text
                tstream.wait_stream(main)
                with torch.cuda.stream(tstream):
                    tf, tl, tp = text_fwd()
                for t in text_in:
                    t.record_stream(tstream)
                if not self.pipelined:
                    main.wait_stream(tstream)
                    for t in (tf, tl, tp):
                        t.record_stream(main)
            else:
                tstream = main
                tf, tl, tp = text_fwd()
            for t in side_in:
                t.record_stream(side)
            if self.pipelined:
                fstream = self._tail
                fstream.wait_stream(tstream)
                fstream.wait_stream(side)
                for t in (sf, sl, sp, imf, il, ip, tf, tl, tp):
                    t.record_stream(fstream)
            else:
                main.wait_stream(side)
                for t in (sf, sl, sp, imf, il, ip):
                    t.record_stream(main)
                fstream = main
        return (sf, sl, sp), (tf, tl, tp), (imf, il, ip), fstream

    def forward_mixed(self, x_speech, ids, mask, gray, present, epilogue=None, text_lens=None):
        """`forward` for a batch of B requests that each have any subset of the modalities. present: host
        flags [B,3] or a bitmask [B] (engine.fusion_mixed_plan); x_speech f32 [ns,56], ids / mask int32
        [nt,128], gray u8 [ni,48,48]: the compact rows of the samples that have each modality, in sample
        order. Each encoder runs once over its rows (not at all when it has none: its outputs are empty
        [0,d] tensors), on the streams `forward` uses; the fusion routes every sample as predict_multimodal
        routes a request (FusionHead.forward_mixed). text_lens: the nt sentence lengths (the packed text
        leg). The serial first-batch autotune rule applies per (text key, ni), the text key nt or (nt, Bp).
        -> the dict `forward` returns with compact per-modality tuples, 'fusion': (fused f64 [B,7], logits,
        attn_w, dec_w) and 'plan'."""
        plan = fusion_mixed_plan(present, True, self.device)
        ns, nt, ni = plan.counts
        for name, t, n in (('x_speech', x_speech, ns), ('ids', ids, nt), ('mask', mask, nt), ('gray', gray, ni)):
            if not isinstance(t, torch.Tensor) or t.dim() < 1 or int(t.shape[0]) != n:
                raise ValueError(f'{name}: expected a tensor of {n} rows (the samples `present` gives this modality)')
        if text_lens is None:
            text_fwd, tkey = (lambda: self.text.forward(ids, mask)), nt
        else:
            text_lens = np.ascontiguousarray(text_lens, dtype=np.int32)
            tkey = (nt, self.text.pack_plan(text_lens)[2])
            text_fwd = lambda: self.text.forward_packed(ids, mask, text_lens)  # noqa: E731
        empty = lambda d: lambda: (self.speech._empty(0, d), self.speech._empty(0, 7), self.speech._empty(0, 7))  # noqa: E731
        s, t, i, fstream = self._encoders(
            (tkey, ni), self._tuned_mixed,
            (lambda: self.speech.forward(x_speech)) if ns else empty(64), text_fwd if nt else empty(768),
            (lambda: self.image.forward(gray)) if ni else empty(512), (x_speech, gray), (ids, mask))
        with torch.cuda.stream(fstream):
            out = {'speech': s, 'text': t, 'image': i, 'fusion': self._fuse_mixed(plan, s, t, i), 'plan': plan}
            extra = epilogue(out) if epilogue is not None else None
        self._record(out, ids, mask, gray, text_lens)
        return out if epilogue is None else (out, extra)

    def _fuse_mixed(self, plan, s, t, i):
        pair = lambda o, n: (o[0], o[2]) if n else None  # noqa: E731
        return self.fusion.forward_mixed(plan, *(pair(o, n) for o, n in zip((s, t, i), plan.counts)))

    def calibrate_image(self, gray):
        """`ImageEncoder.calibrate` on the image encoder (fp32x3 pipelines): gray u8 [B,48,48], or a list of
        such batches. The re-created handle has an empty autotune cache, so the serial first-batch rule starts
        over: the next batch of every size runs serially again. -> {tensor name: (observed max |x|, s)}."""
        res = self.image.calibrate(gray)
        self._tuned.clear()
        self._tuned_mixed.clear()
        return res

    def wait(self, stream=None):
        """Make `stream` (default: the current one) wait for the last batch's fusion."""
        if self.pipelined:
            (stream or torch.cuda.current_stream(self.device)).wait_stream(self._tail)

    def check(self):
        """Synchronize the device, then check every handle (mec_model_check): raise MecError for an
        after-the-fact kernel error. An fp32x3 range trip of the text or image handle is answered instead
        of raised when one batch ran since the last check: that encoder is re-run on its fp32 twin, its
        outputs and the fusion's are overwritten in place in the dict `forward` returned (an `epilogue`'s
        results, computed before, are not), and the handle is re-created with more plane headroom
        (HipModel.recover). With several batches since the last check a trip raises X3RangeError (it
        cannot say which batch). Returns the modalities that were re-run."""
        torch.cuda.synchronize(self.device)
        last, n, redo = self._last, self._since_check, []
        self._since_check = 0
        for name, m in (('text', self.text), ('image', self.image)):
            if last is not None and n == 1 and m.precision == 'fp32x3':
                if m.recover(last.get(name + '_method', 'forward'), last[name], last['out'][name]):
                    redo.append(name)
            else:
                m.check()
        self.speech.check()
        self.fusion.check()
        if redo:
            o = last['out']
            (sf, _, sp), (tf, _, tp), (imf, _, ip) = o['speech'], o['text'], o['image']
            again = (self._fuse_mixed(o['plan'], o['speech'], o['text'], o['image']) if 'plan' in o
                     else self.fusion.forward(sf, tf, imf, sp, tp, ip))
            for d, r in zip(o['fusion'], again):
                d.copy_(r)
            torch.cuda.synchronize(self.device)
        return redo

    @staticmethod
    def pack_rows(out) -> torch.Tensor:
        sp, tp, ip = out['speech'][2], out['text'][2], out['image'][2]
        _, fp, aw, dw = out['fusion']
        return torch.cat([sp, tp, ip, fp, aw, dw], dim=1)

    def models(self):
        return [self.speech, self.text, self.image, self.fusion]

    def set_option(self, key: str, value: int):
        """Set a tuning knob on every handle of the pipeline that knows it."""
        for m in self.models():
            m.set_option(key, value)


def to_device(a: np.ndarray, device) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if not a.flags.writeable:
        a = a.copy()
    return torch.from_numpy(a).to(device)
