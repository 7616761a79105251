"""float64 numpy restatement of the BiLSTM text model (Keras semantics), the reference the text-LSTM
tests compare the HIP kernels with.

Keras LSTM (implementation 1 and 2 agree at inference): z = x.W + h.U + b with gate columns
i | f | c | o; i, f, o = sigmoid, g = tanh; c = f c + i g; h = o tanh(c); h0 = c0 = 0.
Bidirectional runs the backward layer over the reversed sequence and, with return_sequences,
reverses its outputs back to time order before concatenating forward | backward; without, it
concatenates the two final states (the backward one is the state after t = 0).
"""
import numpy as np


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_seq(xz, U, reverse=False):
    """xz [B,L,4u] = x.W + b (hoisted), U [u,4u] -> (y_seq [B,L,u] in time order, h_last [B,u])."""
    xz = np.asarray(xz, np.float64)
    U = np.asarray(U, np.float64)
    B, L, _ = xz.shape
    u = U.shape[0]
    h = np.zeros((B, u))
    c = np.zeros((B, u))
    y = np.zeros((B, L, u))
    for t in (range(L - 1, -1, -1) if reverse else range(L)):
        z = xz[:, t] + h @ U
        i, f, g, o = sigmoid(z[:, :u]), sigmoid(z[:, u:2 * u]), np.tanh(z[:, 2 * u:3 * u]), sigmoid(z[:, 3 * u:])
        c = f * c + i * g
        h = o * np.tanh(c)
        y[:, t] = h
    return y, h


def bidirectional(w, prefix, x, sequences):
    """x [B,L,in] -> [B,L,2u] (sequences) or [B,2u] (final states), forward | backward."""
    outs = []
    for d in ('forward', 'backward'):
        p = f'{prefix}/{d}_lstm/'
        W, U, b = (np.asarray(w[p + k], np.float64) for k in ('kernel', 'recurrent_kernel', 'bias'))
        y, h = lstm_seq(x @ W + b, U, reverse=d == 'backward')
        outs.append(y if sequences else h)
    return np.concatenate(outs, axis=-1)


def forward(w, ids):
    """ids int [B,L] (clamped to the vocabulary like the kernel) -> (feat [B,64], logits [B,7], probs [B,7])."""
    E = np.asarray(w['embedding/embeddings'], np.float64)
    ids = np.clip(np.asarray(ids, np.int64), 0, E.shape[0] - 1)
    x = E[ids]
    y1 = bidirectional(w, 'bidirectional', x, True)
    h2 = bidirectional(w, 'bidirectional_1', y1, False)
    d = lambda n: (np.asarray(w[n + '/kernel'], np.float64), np.asarray(w[n + '/bias'], np.float64))
    (W1, b1), (W2, b2), (W3, b3) = d('dense'), d('dense_1'), d('output')
    a1 = np.maximum(h2 @ W1 + b1, 0.0)
    feat = np.maximum(a1 @ W2 + b2, 0.0)
    logits = feat @ W3 + b3
    e = np.exp(logits - logits.max(1, keepdims=True))
    return feat, logits, e / e.sum(1, keepdims=True)
