"""
Image inference (ResNet50 + 2048->512->7 head) on the MI355X HIP path — drop-in for the
reference's inference/image_inference.py (same class, methods, result dicts, fallback).

The reference transform Resize((224,224)) -> ToTensor -> Normalize (:28-32) and the network
run on the GPU (csrc/resnet.hip): a 48x48 grayscale FER2013 face is resized by a PIL-exact
HIP kernel; any other image is decoded and resized by PIL on the host (the same call
torchvision makes) and uploaded as u8 224x224, gray (1 channel) or RGB (3 channels). The
labels are Config.EMOTIONS[argmax] exactly like the reference (:121-123), including its
class-order quirk against ImageFolder's alphabetical training order.

With resize='gpu' (opt-in) the host keeps the decoding, the RGB conversion and the gray test, and an image of
any size inside mec.image.resize_on_gpu's domain is uploaded as it is and resized on the GPU to PIL's bytes
(csrc/resize.hip), so the results equal resize='host''s bit for bit; predict_arrays / extract_features_arrays
take a batch of in-memory u8 arrays of any sizes.

With convert='gpu' (opt-in, needs resize='gpu') the host keeps only the decoding: an image of mode L, LA, RGB,
RGBA or P inside that domain is uploaded in its native pixel format, and the RGB conversion, the gray test and
the channel selection run on the GPU as well (csrc/image_canon.hip, engine.ingest_ragged), again with 'host''s
bytes; every other mode or size takes the path above.

With decode='gpu' (opt-in, needs convert='gpu') the host does not decode either: a baseline JPEG file inside
mec.jpeg.probe's domain is uploaded as its bytes and decoded on the GPU (csrc/jpeg.hip, engine.ingest_ragged_files)
to Pillow's pixels, so the results equal decode='host''s bit for bit; every other file (PNG, progressive or CMYK
JPEG, ...) and a file the kernels give up is decoded by Pillow as above. predict_files / extract_features_files
take a batch of files at every setting.

Added beyond the reference: predict_array(u8 image) and predict_batch(u8 [B,48,48]), and
`backbone='mobilenet_v2'` (README.md:13 names MobileNetV2 as the image model; the reference
code builds ResNet50): the same transform, head, feature and result dicts on a
torchvision-mobilenet_v2 backbone (csrc/mobilenet.hip; parity unpinned, no reference code).
"""

import io
from typing import Dict

import numpy as np

from config import Config
from mec import checkpoints, engine, jpeg as _jpeg
from mec._lib import MecError
from mec.image import MODEL_SHAPES, PIX_L, PIX_RGB, native_pixels, resize_on_gpu


def _route(image, resize: str = 'host'):
    """PIL image -> (u8 array [H,W,C], ragged). ragged False: the array has one of the shapes the HIP path
    takes, (48,48,1) or PIL-resized (224,224,C). ragged True (resize='gpu' only): the image's own pixels,
    gray (C = 1) or RGB (C = 3), to be resized on the GPU (engine.resize_ragged); only an image inside
    mec.image.resize_on_gpu's domain is routed there. The gray test runs on the original pixels either way."""
    from PIL import Image
    rgb = image.convert('RGB')  # reference :112
    a = np.asarray(rgb, dtype=np.uint8)
    gray = bool((a[..., 0] == a[..., 1]).all() and (a[..., 0] == a[..., 2]).all())
    if gray and a.shape[:2] == (48, 48):
        return np.ascontiguousarray(a[..., :1]), False  # GPU resize path
    if resize == 'gpu' and resize_on_gpu(a.shape[0], a.shape[1]):
        return np.ascontiguousarray(a[..., :1] if gray else a), True
    r = np.asarray(rgb.resize((224, 224), Image.BILINEAR), dtype=np.uint8)  # Resize((224,224))
    return np.ascontiguousarray(r[..., :1] if gray else r), False


def _as_image(arr):
    """u8 array [H,W] / [H,W,1] (gray) or [H,W,3] (RGB) -> PIL image."""
    from PIL import Image
    a = np.asarray(arr, np.uint8)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[..., 0]
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise ValueError(f'image array: shape {a.shape} is not [H,W], [H,W,1] or [H,W,3]')
    return Image.fromarray(np.ascontiguousarray(a), 'L' if a.ndim == 2 else 'RGB')


def plan_batches(made):
    """made: per item of a `forward_routed` list, (its model-input shape, whether the device makes it) ->
    {shape: (rows, device slots, host slots)} for the three shapes: the shape's rows in ascending order, which is
    its forward's batch, and where in that batch the device-made and the host-made rows stand, each ascending (the
    order in which either part holds its rows)."""
    plan = {shape: ([], [], []) for shape in MODEL_SHAPES}
    for row, (shape, on_device) in enumerate(made):
        rows, dev_at, host_at = plan[tuple(shape)]
        (dev_at if on_device else host_at).append(len(rows))
        rows.append(row)
    return plan


class Native(tuple):
    """(pixels as decoded, mec.image.PIX_* format, palette or None): an image that convert='gpu' hands to
    engine.ingest_ragged unconverted, where a `_route` result would stand."""


_KINDS = {'resnet50': 'image', 'mobilenet_v2': 'image_mbv2'}


class ImageInference:
    def __init__(self, weights=None, seed=None, device=None, backbone='resnet50', precision=None, resize='host',
                 convert='host', decode='host'):
        if backbone not in _KINDS:
            raise ValueError(f'backbone must be one of {sorted(_KINDS)}')
        if resize not in ('host', 'gpu'):
            raise ValueError("resize must be 'host' or 'gpu'")
        if convert not in ('host', 'gpu'):
            raise ValueError("convert must be 'host' or 'gpu'")
        if convert == 'gpu' and resize != 'gpu':
            raise ValueError("convert='gpu' requires resize='gpu'")
        if decode not in ('host', 'gpu'):
            raise ValueError("decode must be 'host' or 'gpu'")
        if decode == 'gpu' and not (resize == 'gpu' and convert == 'gpu'):
            raise ValueError("decode='gpu' requires resize='gpu' and convert='gpu'")
        # 'gpu': a baseline JPEG file inside mec.jpeg.probe's domain is uploaded undecoded and decoded on the GPU
        # (csrc/jpeg.hip) to Pillow's pixels, so with 'host''s results bit for bit; every other file is decoded by
        # Pillow as with 'host'
        self.decode = decode
        # 'gpu': an image of mode L, LA, RGB, RGBA or P inside the GPU resize's domain is uploaded as decoded; the
        # RGB conversion, the gray test and the channel selection run there too (csrc/image_canon.hip), with
        # 'host''s bytes and so with its results bit for bit
        self.convert = convert
        # 'gpu': an image that is not a 48x48 gray face and lies in the GPU resize's domain is uploaded as it
        # is and resized there (csrc/resize.hip), with PIL's bytes and so with 'host''s results bit for bit
        self.resize = resize
        self.emotions = Config.EMOTIONS
        self.backbone = backbone
        self.model = None
        w = checkpoints.resolve(_KINDS[backbone], weights, seed)
        if w is not None:  # raises MecError without HIP/GPU
            self.model = engine.IMAGE_BACKBONES[backbone](w, device=device,
                                                          precision=checkpoints.precision(precision))
        self.device = self.model.device if self.model is not None else None

    def _fallback(self) -> Dict:
        probs = np.ones(len(self.emotions)) * (0.1 / (len(self.emotions) - 1))
        idx = self.emotions.index('neutral')
        probs[idx] = 0.9
        return {'emotion': 'neutral', 'confidence': float(probs[idx]), 'all_probabilities': probs.tolist()}

    def _forward(self, arr: np.ndarray):
        x = engine.to_device(np.asarray(arr, np.uint8)[None], self.device)
        # synchronized and checked: an fp32x3 batch whose activations leave the planes' range is re-run on
        # the fp32 engine (engine.HipModel.recover), never answered with NaN probs
        feat, logits, probs = self.model.checked('forward_u8', x)
        return feat.cpu().numpy()[0], probs.cpu().numpy()[0]

    def _device_parts(self, rows, pixels, ingest):
        """The device-made rows of a `forward_routed` list -> {model-input shape: (u8 batch on the device, its
        rows, ascending)}, and the rows of the files the GPU decoder gave up. `pixels` are
        engine.ingest_ragged_files items. ingest True (the list holds a `Native` or a file): one
        engine.ingest_ragged_files call; False (L or RGB pixels only): one engine.resize_ragged call per channel
        count."""
        if ingest:
            _, groups, status = engine.ingest_ragged_files(pixels, self.device)
            return ({shape: (x, [rows[j] for j in local]) for shape, (x, local) in zip(MODEL_SHAPES, groups)},
                    [rows[j] for j in np.flatnonzero(status)])
        parts = {}
        for C in (1, 3):
            local = [j for j, px in enumerate(pixels) if px[0].shape[2] == C]
            if local:
                parts[(224, 224, C)] = (engine.resize_ragged([pixels[j][0] for j in local], self.device),
                                        [rows[j] for j in local])
        return parts, []

    def forward_routed(self, items, unreadable=None):
        """items: a list of `route` results and undecoded files (mec.jpeg.Blob, decode='gpu') -> (feat [n,512],
        probs [n,7]) device tensors in the list's order. A file the GPU decoder gives up is decoded by Pillow and
        takes the host route; what Pillow raises for it is raised, or with a dict `unreadable` stored there by row
        (that row's results are zero).
        One forward per model-input shape, (48,48,1) / (224,224,1) / (224,224,3), as a batch of PIL-resized
        images is grouped: the rows made on the device (`_device_parts`: `Native` items and `_route` results
        still to be resized) stand in their shape's batch where the host's results would, in ascending row order
        (`plan_batches`), so every setting of `resize` and `convert` runs the same forwards on the same bytes."""
        import torch
        dev = self.device
        at = lambda rows: torch.tensor(rows, dtype=torch.int64, device=dev)  # noqa: E731
        host, drows, pixels = {}, [], []  # row -> host-made array; the device-made rows and their pixels
        for row, it in enumerate(items):
            if isinstance(it, Native):
                pixels.append(tuple(it))
            elif isinstance(it, _jpeg.Blob):
                pixels.append(it)
            elif it[1]:
                pixels.append((it[0], PIX_L if it[0].shape[2] == 1 else PIX_RGB, None))
            else:
                host[row] = it[0]
                continue
            drows.append(row)
        parts, given_up = self._device_parts(drows, pixels, any(isinstance(it, (Native, _jpeg.Blob)) for it in items))
        for row in given_up:
            try:
                host[row] = self._host_pixels(items[row].data)
            except MecError:
                raise
            except Exception as e:
                if unreadable is None:
                    raise
                unreadable[row] = e
                host[row] = np.zeros((224, 224, 1), np.uint8)
        made = {row: (a.shape, False) for row, a in host.items()}
        made.update((row, (shape, True)) for shape, (_, prows) in parts.items() for row in prows)
        feat = torch.empty((len(items), 512), dtype=torch.float32, device=dev)
        probs = torch.empty((len(items), 7), dtype=torch.float32, device=dev)
        for shape, (rows, dev_at, host_at) in plan_batches([made[row] for row in range(len(items))]).items():
            if not rows:
                continue
            x = parts[shape][0] if dev_at else None
            if host_at:
                h = engine.to_device(np.stack([host[rows[k]] for k in host_at]), dev)
                if dev_at:  # a part that is the whole batch is used as it is
                    x, part = torch.empty((len(rows),) + shape, dtype=torch.uint8, device=dev), x
                    x.index_copy_(0, at(dev_at), part)
                    x.index_copy_(0, at(host_at), h)
                else:
                    x = h
            f, _, p = self.model.checked('forward_u8', x)
            feat.index_copy_(0, at(rows), f)
            probs.index_copy_(0, at(rows), p)
        return feat, probs

    @staticmethod
    def _host_pixels(data):
        """A file's bytes -> the host-made model input, as resize='host' makes it (PIL's bytes are the GPU's)."""
        from PIL import Image
        with Image.open(io.BytesIO(data)) as im:
            return _route(im, 'host')[0]

    def _convert_on_gpu(self) -> bool:
        return self.convert == 'gpu' and self.resize == 'gpu'

    def route(self, image):
        """PIL image -> an item of `forward_routed`: with convert='gpu' a `Native` for an image the GPU ingest
        covers (mec.image.native_pixels: no conversion and no gray test on the host), else `_route`'s result."""
        if self._convert_on_gpu():
            native = native_pixels(image)
            if native is not None:
                return Native(native)
        return _route(image, self.resize)

    def route_array(self, arr):
        """u8 array [H,W] / [H,W,1] / [H,W,3] -> an item of `forward_routed`; with convert='gpu' an array inside
        the GPU resize's domain goes on as L / RGB pixels without a PIL image being built."""
        if not self._convert_on_gpu():
            return _route(_as_image(arr), self.resize)
        a = np.asarray(arr, np.uint8)
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[..., 0]
        if a.ndim in (2, 3) and (a.ndim == 2 or a.shape[2] == 3) and resize_on_gpu(a.shape[0], a.shape[1]):
            return Native((a, PIX_L if a.ndim == 2 else PIX_RGB, None))
        return _route(_as_image(a), self.resize)  # raises for a shape that is no image's

    def _forward_image(self, image):
        item = self.route(image)
        if isinstance(item, Native) or item[1]:
            feat, probs = self.forward_routed([item])
            return feat.cpu().numpy()[0], probs.cpu().numpy()[0]
        return self._forward(item[0])

    @staticmethod
    def _as_dict(emotions, probs: np.ndarray) -> Dict:
        idx = int(np.argmax(probs))
        return {'emotion': emotions[idx], 'confidence': float(probs[idx]), 'all_probabilities': probs.tolist()}

    def predict_array(self, arr) -> Dict:
        """u8 image [48,48] / [48,48,1] / [224,224,1] / [224,224,3] -> result dict."""
        a = np.asarray(arr, np.uint8)
        if a.ndim == 2:
            a = a[..., None]
        return self._as_dict(self.emotions, self._forward(a)[1])

    def extract_features_arrays(self, arrays):
        """u8 images of any sizes, [H,W] / [H,W,1] gray or [H,W,3] RGB -> (feat [n,512], probs [n,7]) numpy,
        each image treated as `extract_features` treats a file that decodes to it (RGB conversion, gray test,
        Resize((224,224))), the batch run as one forward per model-input shape. With resize='gpu' the images
        of the GPU resize's domain are uploaded unresized in one copy and resized there; with convert='gpu' they are
        not converted or compared on the host either (`route_array`)."""
        if self.model is None:
            raise RuntimeError('image model not loaded')
        items = [self.route_array(a) for a in arrays]
        if not items:
            return np.zeros((0, 512), np.float32), np.zeros((0, 7), np.float32)
        feat, probs = self.forward_routed(items)
        return feat.cpu().numpy(), probs.cpu().numpy()

    def predict_arrays(self, arrays):
        """`extract_features_arrays`' probabilities as one result dict per image."""
        return [self._as_dict(self.emotions, p) for p in self.extract_features_arrays(arrays)[1]]

    def file_item(self, path):
        """An image file -> its `forward_routed` item; raises what Pillow raises for a file it cannot read. With
        decode='gpu' the file is read once: a JPEG of the GPU decoder's domain goes on undecoded (mec.jpeg.probe),
        every other file is opened by Pillow from the same bytes."""
        from PIL import Image
        if self.decode == 'gpu':
            with open(path, 'rb') as f:
                data = f.read()
            blob = _jpeg.probe(data)
            if blob is not None:
                return blob
            with Image.open(io.BytesIO(data)) as im:
                return self.route(im)
        with Image.open(path) as im:
            return self.route(im)

    def _forward_files(self, paths, unreadable):
        """-> (feat [n,512], probs [n,7]) numpy; the rows Pillow cannot read are zero and stored in `unreadable`."""
        items = []
        for row, p in enumerate(paths):
            try:
                items.append(self.file_item(p))
            except MecError:
                raise
            except Exception as e:
                unreadable[row] = e
                items.append((np.zeros((224, 224, 1), np.uint8), False))
        if not items:
            return np.zeros((0, 512), np.float32), np.zeros((0, 7), np.float32)
        feat, probs = self.forward_routed(items, unreadable)
        return feat.cpu().numpy(), probs.cpu().numpy()

    def extract_features_files(self, paths):
        """Image files -> (feat [n,512], probs [n,7]) numpy, each file treated as `extract_features` treats it,
        the batch run as one forward per model-input shape; raises what Pillow raises for a file it cannot read.
        With decode='gpu' the JPEG files of the GPU decoder's domain are uploaded undecoded in one copy and
        decoded, converted and resized there."""
        if self.model is None:
            raise RuntimeError('image model not loaded')
        unreadable = {}
        feat, probs = self._forward_files(list(paths), unreadable)
        for row in sorted(unreadable):
            raise unreadable[row]
        return feat, probs

    def predict_files(self, paths):
        """`predict` for a batch of files: one result dict per file, the fallback for a file Pillow cannot read."""
        paths = list(paths)
        if self.model is None:
            return [self._fallback() for _ in paths]
        unreadable = {}
        probs = self._forward_files(paths, unreadable)[1]
        for row in sorted(unreadable):
            print(f"Image inference error: {unreadable[row]}")
        return [self._fallback() if row in unreadable else self._as_dict(self.emotions, p) for row, p in enumerate(probs)]

    def predict(self, image_file_path: str) -> Dict:
        if self.model is None:
            return self._fallback()
        if self.decode == 'gpu':
            return self.predict_files([image_file_path])[0]
        try:
            from PIL import Image
            with Image.open(image_file_path) as im:
                feat_probs = self._forward_image(im)
            return self._as_dict(self.emotions, feat_probs[1])
        except MecError:
            raise  # a failing HIP kernel is never hidden behind the fallback
        except Exception as e:
            print(f"Image inference error: {e}")
            return self._fallback()

    def extract_features(self, image_file_path: str):
        """(512-d fc[2] feature, 7 probs) — one forward instead of three."""
        if self.model is None:
            return None, None
        if self.decode == 'gpu':
            feat, probs = self.extract_features_files([image_file_path])
            return feat[0], probs[0]
        from PIL import Image
        with Image.open(image_file_path) as im:
            return self._forward_image(im)

    def calibrate(self, gray_batch):
        """fp32x3 only: set the model's activation-plane exponents from an observed batch instead of the BatchNorm
        estimate (engine.ImageEncoder.calibrate). gray_batch: device u8 [B,48,48] (or [B,H,W,C] as forward_u8 takes
        it), or a list of such batches, representative of the data. -> {tensor name: (observed max |x|, exponent)}."""
        if self.model is None:
            raise RuntimeError('image model not loaded')
        return self.model.calibrate(gray_batch)

    def predict_batch(self, gray):
        """gray: device u8 [B,48,48] -> (feat [B,512], logits [B,7], probs [B,7]). Asynchronous on the
        current stream, except on an fp32x3 handle: there it synchronizes and checks, so a batch outside
        the planes' range is answered by the fp32 engine (engine.HipModel.checked)."""
        if self.model is None:
            raise RuntimeError('image model not loaded')
        if self.model.precision == 'fp32x3':
            return self.model.checked('forward', gray)
        return self.model.forward(gray)
