"""Trained-like weights for the encoder tests (a helper module, imported by the tests that need it).

transformers' default initialisation gives every Linear bias 0, every LayerNorm weight 1 and bias 0, and N(0, 0.02) Linear
weights: attention softmaxes are nearly uniform and the LayerNorm the hand-written encoder folds into the next Linear
(csrc/encoder_small.hpp, enc_fold_ln_kernel) reduces to the identity. `roughen` overwrites such a module, in place and
deterministically, with weights that have a trained encoder's STRUCTURE: non-zero biases, LayerNorm weights around 1 with a few
outlier channels, LayerNorm biases with a non-zero mean, peaked attention heads, GELU inputs out to about +-4 and a token
classifier with clear argmaxes. Every tensor is drawn on its own (distinct per layer and per Q / K / V).

Profiles:
  "trained": the above; the pre-norm rows of every LayerNorm keep |row mean| / row std below about 0.5.
  "offset":  a per-channel offset on the word embeddings and a LayerNorm bias mean large enough that most tokens reach
             |row mean| / row std >= 2 at every LayerNorm - the stress case of the folded LayerNorm, whose rounding error grows
             with that ratio.
"""
import torch

PROFILES = ("trained", "offset")


def encoder_of(module):
    """-> (the BertModel-like encoder, the token classifier or None) of a BertModel / (XLM)RobertaModel or a *ForTokenClassification"""
    for name in ("bert", "roberta"):
        inner = getattr(module, name, None)
        if inner is not None:
            return inner, getattr(module, "classifier", None)
    return module, None


@torch.no_grad()
def roughen(module, seed: int, profile: str = "trained"):
    """Overwrite the parameters of `module` in place (whatever its device and dtype) with trained-like values; returns it."""
    if profile not in PROFILES:
        raise ValueError(f"profile {profile!r}: one of {PROFILES}")
    bert, clf = encoder_of(module)
    cfg = bert.config
    H, nh = int(cfg.hidden_size), int(cfg.num_attention_heads)
    dh = H // nh
    gen = torch.Generator().manual_seed(int(seed))
    offset = profile == "offset"

    def normal(shape, std, mean=0.0):
        return torch.randn(shape, generator=gen, dtype=torch.float64) * std + mean

    def put(p, value):
        p.copy_(value.to(dtype=p.dtype, device=p.device))

    def centred(w):
        # "offset": the rows of a Linear that reads a LayerNorm's output (or GELU's) sum to 0, as if training had taught it to
        # ignore the common offset - which otherwise passes through it as a large per-channel constant, pushes every softmax to
        # one-hot and re-inflates the next LayerNorm's row spread until no row keeps a large |mean| / std
        return w - w.mean(1, keepdim=True) if offset else w

    def layer_norm(ln):
        n = ln.weight.shape[0]
        g = normal(n, 0.15, 1.0)
        pick = torch.randperm(n, generator=gen)[:2 + int(torch.randint(0, 3, (1,), generator=gen))]   # 2-4 outlier channels
        mag = 3.0 + 5.0 * torch.rand(len(pick), generator=gen, dtype=torch.float64)
        mag[0] = -mag[0]                                                                              # one of them negative
        g[pick] = mag
        put(ln.weight, g)
        # a non-zero mean: small in "trained"; in "offset" large against the unit spread of a normalised row
        put(ln.bias, normal(n, 0.1, 4.0 if offset else 0.05))

    emb = bert.embeddings
    V = emb.word_embeddings.weight.shape[0]
    word = normal((V, H), 0.04)
    if offset:
        word += normal(H, 0.03, 0.2)        # per channel: most rows' mean is several times their spread
    put(emb.word_embeddings.weight, word)
    put(emb.position_embeddings.weight, normal(emb.position_embeddings.weight.shape, 0.03))
    put(emb.token_type_embeddings.weight, normal(emb.token_type_embeddings.weight.shape, 0.05))
    layer_norm(emb.LayerNorm)

    for layer in bert.encoder.layer:
        a = layer.attention.self
        # attention logits q.k / 8 with std ~4 (std of q and k per element ~2 over 64 dims); two heads per layer sharper still,
        # nearly one-hot
        head = torch.ones(nh, dtype=torch.float64)
        head[torch.randperm(nh, generator=gen)[:2]] = 1.6
        rows = head.repeat_interleave(dh)[:, None]
        put(a.query.weight, centred(normal((H, H), 0.07) * rows))
        put(a.key.weight, centred(normal((H, H), 0.07) * rows))
        put(a.value.weight, centred(normal((H, H), 0.03)))
        put(a.query.bias, normal(H, 0.1))
        put(a.key.bias, normal(H, 0.1))
        put(a.value.bias, normal(H, 0.08))
        o = layer.attention.output
        put(o.dense.weight, normal(o.dense.weight.shape, 0.03))
        put(o.dense.bias, normal(H, 0.07))
        layer_norm(o.LayerNorm)
        up = layer.intermediate.dense
        put(up.weight, centred(normal(up.weight.shape, 0.06)))           # GELU inputs with std ~1.7: out to about +-4 and beyond
        put(up.bias, normal(up.bias.shape, 0.1))
        down = layer.output.dense
        put(down.weight, centred(normal(down.weight.shape, 0.02)))
        put(down.bias, normal(H, 0.07))
        layer_norm(layer.output.LayerNorm)

    if clf is not None:
        L = clf.weight.shape[0]
        put(clf.weight, normal((L, H), 0.1))                   # logits with std ~3: most argmaxes clear
        put(clf.bias, normal(L, 0.5))
    return module
