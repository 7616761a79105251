"""Offline converter: the reference's trained Keras BiLSTM text model (.h5) -> text_lstm_weights.npz.

The reference trains the model with TensorFlow 2.13 (requirements.txt:6) and saves it through
ModelCheckpoint(Config.TEXT_MODEL_PATH) (model_training/train_lstm_text_model.py:187), i.e. the
Keras-2 legacy HDF5 layout:

    /model_weights                 attrs: layer_names = [b'embedding', b'bidirectional', ...]
    /model_weights/<layer>         attrs: weight_names = [b'bidirectional/forward_lstm/lstm_cell_1/kernel:0', ...]

The network (train_lstm_text_model.py:96-120) is Embedding, SpatialDropout1D, two Bidirectional
LSTMs, then Dense / Dropout / Dense / Dropout / Dense. This tool walks `layer_names` in order, keeps
the layers that own weights and classifies them by their weight names, so Keras' auto-numbered layer
and cell names (bidirectional_3, lstm_cell_7, ...) do not matter: `embeddings` = Embedding; six
tensors whose paths name a forward and a backward layer = Bidirectional LSTM (kernel,
recurrent_kernel, bias each); kernel + bias = Dense. Output names are those of
mec.synthetic.text_lstm_spec(). The embedding keeps its trained row count (vocab_size =
min(10000, len(word_index) + 1), :171); the loader zero-pads it to 10000 rows.

The tokenizer is a pickle in the reference (`_tokenizer.pkl`) and is NOT read here or anywhere in
this repo. Export it once, in the environment that trained it:

    python -c "import pickle; t = pickle.load(open('models/text_model_tokenizer.pkl', 'rb')); \
               open('models/text_lstm_tokenizer.json', 'w').write(t.to_json())"

Needs h5py + numpy. Unpinned: no TensorFlow-written file is available to this repo's tests, which
cover the spec, the loader and the arithmetic (tests/test_text_lstm_oracle.py).

    python tools/convert_text_lstm_h5.py models/text_model.h5 -o models/text_lstm_weights.npz
"""
import argparse
import sys

import numpy as np

UNITS = (128, 64)
DENSE = ('dense', 'dense_1', 'output')


def _s(x):
    return x.decode() if isinstance(x, bytes) else str(x)


def read_layers(path):
    """[(kind, {name: array})] for every weighted layer, in model order. LSTM tensors are keyed
    '<forward|backward>/<kernel|recurrent_kernel|bias>'."""
    import h5py
    out = []
    with h5py.File(path, 'r') as f:
        g = f['model_weights'] if 'model_weights' in f else f  # save_weights() files have no wrapper
        for lname in [_s(n) for n in g.attrs['layer_names']]:
            lg = g[lname]
            wnames = [_s(n) for n in lg.attrs.get('weight_names', [])]
            if not wnames:
                continue
            ws = {}
            for wn in wnames:
                parts = wn.split(':')[0].split('/')
                short = parts[-1]
                d = next((k for k in ('forward', 'backward') if any(p.startswith(k) for p in parts[:-1])), None)
                ws[f'{d}/{short}' if d else short] = np.asarray(lg[wn], dtype=np.float32)
            if set(ws) == {'embeddings'}:
                out.append(('embedding', ws))
            elif set(ws) == {f'{d}/{k}' for d in ('forward', 'backward') for k in ('kernel', 'recurrent_kernel', 'bias')}:
                out.append(('bilstm', ws))
            elif set(ws) == {'kernel', 'bias'}:
                out.append(('dense', ws))
            else:
                raise ValueError(f'{path}: layer {lname} has unexpected weights {sorted(ws)}')
    return out


def convert(h5_path):
    layers = read_layers(h5_path)
    kinds = [k for k, _ in layers]
    want = ['embedding', 'bilstm', 'bilstm', 'dense', 'dense', 'dense']
    if kinds != want:
        raise ValueError(f'{h5_path}: weighted layers {kinds}, expected {want} (train_lstm_text_model.py:96-120)')
    out = {'embedding/embeddings': layers[0][1]['embeddings']}
    emb = out['embedding/embeddings']
    if emb.ndim != 2 or emb.shape[1] != 128 or not 1 <= emb.shape[0] <= 10000:
        raise ValueError(f'embedding has shape {emb.shape}, expected [<= 10000, 128]')
    fin = 128
    for li, u in enumerate(UNITS):
        p = 'bidirectional' + ('' if li == 0 else f'_{li}')
        for d in ('forward', 'backward'):
            shapes = {'kernel': (fin, 4 * u), 'recurrent_kernel': (u, 4 * u), 'bias': (4 * u,)}
            for k, sh in shapes.items():
                a = layers[1 + li][1][f'{d}/{k}']
                if a.shape != sh:
                    raise ValueError(f'{p}/{d}_lstm/{k} has shape {a.shape}, expected {sh}')
                out[f'{p}/{d}_lstm/{k}'] = a
        fin = 2 * u
    for name, (_, ws), fo in zip(DENSE, layers[3:], (128, 64, 7)):
        if ws['kernel'].shape != (fin, fo) or ws['bias'].shape != (fo,):
            raise ValueError(f'{name}/kernel has shape {ws["kernel"].shape}, expected {(fin, fo)}')
        out[f'{name}/kernel'], out[f'{name}/bias'] = ws['kernel'], ws['bias']
        fin = fo
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('h5')
    ap.add_argument('-o', '--out', required=True)
    a = ap.parse_args(argv)
    w = convert(a.h5)
    np.savez(a.out, **w)
    print(f'wrote {a.out}: {len(w)} arrays, {w["embedding/embeddings"].shape[0]} embedding rows', file=sys.stderr)


if __name__ == '__main__':
    main()
