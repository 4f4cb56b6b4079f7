"""The trained-like weights of tests/encoder_weights.py, in float64 on the CPU (no GPU code involved).

1. Each profile lands in the regime it claims: pre-norm |row mean| / row std at every LayerNorm, peaked attention heads, the
   range of the GELU inputs, clear classifier argmaxes.
2. Sensitivity: every mistake the GPU encoder could make in its folded LayerNorms and borrowed biases - a parameter group left
   at its default-init value, LayerNorm1 and LayerNorm2 swapped, every layer reading layer 0's LayerNorms, the fold's g applied
   along the output axis - moves the float64 unit embedding by >= 1e-3, 100x the GPU tests' tolerance (1e-5): under these
   weights those tests can see each of them. (Under transformers' default init most of them move it by exactly 0.)
"""
import copy

import numpy as np
import pytest
import torch

from encoder_weights import PROFILES, encoder_of, roughen

H, LAYERS, VOCAB = 768, 3, 2000
SEQS = [[101] + [int(t) for t in np.random.default_rng(3).integers(5, VOCAB, n)] + [102] for n in (6, 19, 37)]
MOVE = 1e-3


def _bert(profile=None, seed=11):
    from transformers import BertConfig, BertModel
    cfg = BertConfig(vocab_size=VOCAB, hidden_size=H, num_hidden_layers=LAYERS, num_attention_heads=12, intermediate_size=4 * H,
                     max_position_embeddings=512)
    torch.manual_seed(0)
    m = BertModel(cfg, add_pooling_layer=False).double().eval()
    m.set_attn_implementation("eager")
    return roughen(m, seed, profile) if profile else m


@pytest.fixture(scope="module", params=PROFILES)
def model(request):
    return request.param, _bert(request.param)


def _params(m):
    """the float64 parameters of a BertModel, by the names the GPU encoder's descriptor uses"""
    e = m.embeddings
    P = {"word": e.word_embeddings.weight, "pos": e.position_embeddings.weight, "type0": e.token_type_embeddings.weight[0],
         "emb_ln_g": e.LayerNorm.weight, "emb_ln_b": e.LayerNorm.bias, "layers": []}
    for l in m.encoder.layer:
        a = l.attention.self
        P["layers"].append({
            "w_qkv": torch.cat([a.query.weight, a.key.weight, a.value.weight]), "b_qkv": torch.cat([a.query.bias, a.key.bias, a.value.bias]),
            "w_ao": l.attention.output.dense.weight, "b_ao": l.attention.output.dense.bias,
            "ln1_g": l.attention.output.LayerNorm.weight, "ln1_b": l.attention.output.LayerNorm.bias,
            "w_up": l.intermediate.dense.weight, "b_up": l.intermediate.dense.bias,
            "w_down": l.output.dense.weight, "b_down": l.output.dense.bias,
            "ln2_g": l.output.LayerNorm.weight, "ln2_b": l.output.LayerNorm.bias})
    return P


def _norm_stats(y, eps=1e-12):
    mean = y.mean(-1, keepdim=True)
    var = ((y - mean) ** 2).mean(-1, keepdim=True)
    return mean, torch.rsqrt(var + eps)


@torch.no_grad()
def _forward(P, ids, wrong_axis=False, trace=None):
    """The encoder restated in float64 the way the GPU one computes it: every Linear that reads a LayerNorm's output takes the
    PRE-norm rows y and the LayerNorm folded into its weights, rstd (y (W diag g)^T - mean c1) + c2 (c1 = W g, c2 = W b + bias).
    wrong_axis: the fold's g applied along the output axis instead (W'[n, k] = g[n mod K] W[n, k], c1 = W' 1). trace: a dict
    that collects the pre-norm rows of every LayerNorm, the attention probabilities and the GELU inputs."""
    L = len(ids)
    y = P["word"][torch.tensor(ids)] + P["type0"] + P["pos"][:L]
    g, b = P["emb_ln_g"], P["emb_ln_b"]
    nh, dh = 12, H // 12

    def ln(y, g, b):
        mean, rstd = _norm_stats(y)
        if trace is not None:
            trace.setdefault("prenorm", []).append(((mean.abs() * rstd).squeeze(-1)))
        return (y - mean) * rstd * g + b

    def folded(y, g, b, w, bias):
        mean, rstd = _norm_stats(y)
        K = w.shape[1]
        gk = g[torch.arange(w.shape[0]) % K][:, None] if wrong_axis else g[None, :]
        wg = w * gk
        c1 = wg.sum(1)
        c2 = w @ b + bias
        return rstd * (y @ wg.t() - mean * c1) + c2

    for p in P["layers"]:
        qkv = folded(y, g, b, p["w_qkv"], p["b_qkv"])
        x = ln(y, g, b)                                               # the residual: the normalised row itself
        q, k, v = (qkv[:, i * H:(i + 1) * H].view(L, nh, dh).transpose(0, 1) for i in range(3))
        att = torch.softmax(q @ k.transpose(1, 2) / dh ** 0.5, -1)
        if trace is not None:
            trace.setdefault("attention", []).append(att)
        ctx = (att @ v).transpose(0, 1).reshape(L, H)
        y1 = ctx @ p["w_ao"].t() + p["b_ao"] + x
        pre = folded(y1, p["ln1_g"], p["ln1_b"], p["w_up"], p["b_up"])
        if trace is not None:
            trace.setdefault("gelu_in", []).append(pre)
        x1 = ln(y1, p["ln1_g"], p["ln1_b"])
        y = torch.nn.functional.gelu(pre) @ p["w_down"].t() + p["b_down"] + x1
        g, b = p["ln2_g"], p["ln2_b"]
    return ln(y, g, b)


def _unit_mean(hidden):
    return torch.nn.functional.normalize(hidden.mean(0), dim=0)


def _embed_hf(m, ids):
    with torch.no_grad():
        h = m(input_ids=torch.tensor([ids])).last_hidden_state[0]
    return _unit_mean(h)


def test_the_float64_restatement_equals_transformers_forward(model):
    """the folded-LayerNorm restatement above is the same function as transformers' BertModel (so the wrong-axis mutation
    below is a mutation of the right thing)"""
    profile, m = model
    P = _params(m)
    for ids in SEQS:
        with torch.no_grad():
            want = m(input_ids=torch.tensor([ids])).last_hidden_state[0]
        got = _forward(P, ids)
        assert float((got - want).abs().max()) <= 1e-9 * float(want.abs().max()), profile


def test_default_init_is_the_regime_the_older_tests_covered():
    """what roughen is for: transformers' default init has zero biases and identity LayerNorms"""
    m = _bert(None)
    P = _params(m)
    assert float(P["emb_ln_b"].abs().max()) == 0.0 and float((P["emb_ln_g"] - 1).abs().max()) == 0.0
    for p in P["layers"]:
        for name in ("b_qkv", "b_ao", "b_up", "b_down", "ln1_b", "ln2_b"):
            assert float(p[name].abs().max()) == 0.0, name
        assert float((p["ln1_g"] - 1).abs().max()) == 0.0 and float((p["ln2_g"] - 1).abs().max()) == 0.0


def test_roughen_is_deterministic_and_draws_every_tensor_on_its_own():
    a, b = _bert("trained", seed=5), _bert("trained", seed=5)
    for (n1, p1), (n2, p2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert n1 == n2 and torch.equal(p1, p2), n1
    assert not torch.equal(_bert("trained", seed=6).encoder.layer[0].attention.self.query.weight, a.encoder.layer[0].attention.self.query.weight)
    P = _params(a)
    l0, l1 = P["layers"][0], P["layers"][1]
    for name in ("b_qkv", "b_ao", "b_up", "b_down", "ln1_g", "ln1_b", "ln2_g", "ln2_b"):
        assert not torch.allclose(l0[name], l1[name]), name                       # per layer
    assert not torch.allclose(l0["ln1_g"], l0["ln2_g"]) and not torch.allclose(l0["ln1_b"], l0["ln2_b"])
    bq, bk, bv = l0["b_qkv"].view(3, H)
    assert not torch.allclose(bq, bk) and not torch.allclose(bk, bv)              # per Q / K / V
    for ln_g in [P["emb_ln_g"]] + [p[n] for p in P["layers"] for n in ("ln1_g", "ln2_g")]:
        out = ln_g[(ln_g - 1).abs() > 1.5]
        assert 2 <= len(out) <= 4 and float(out.abs().min()) >= 3 and float(out.abs().max()) <= 8 and int((out < 0).sum()) >= 1
        assert abs(float(ln_g[(ln_g - 1).abs() <= 1.5].std()) - 0.15) <= 0.03


def test_each_profile_lands_in_its_regime(model):
    profile, m = model
    P = _params(m)
    trace = {}
    rng = np.random.default_rng(8)
    for n in (12, 30, 60):
        _forward(P, [101] + [int(t) for t in rng.integers(5, VOCAB, n)] + [102], trace=trace)
    ratios = trace["prenorm"]                                     # per LayerNorm (embeddings, then LN1 / LN2 of every layer), per call
    per_ln = [torch.cat(ratios[i::1 + 2 * LAYERS]) for i in range(1 + 2 * LAYERS)]
    if profile == "trained":
        for i, r in enumerate(per_ln):
            assert float(r.max()) < 0.5, (i, float(r.max()))
    else:
        for i, r in enumerate(per_ln):
            print(f"LayerNorm {i}: {float((r >= 2).double().mean()):.2f} of tokens at |mean| / std >= 2")
            assert float((r >= 2).double().mean()) >= 0.10, (i, float((r >= 2).double().mean()))
    # attention: some heads nearly one-hot (mean entropy per query row well under one nat), none left near-uniform
    # (entropy as a fraction of the uniform distribution's, log L, over the calls of 32 and 62 tokens)
    ent = [-(a * torch.log(a.clamp_min(1e-300))).sum(-1).mean(-1) / np.log(a.shape[-1]) for a in trace["attention"] if a.shape[-1] >= 30]
    ent = torch.cat(ent)
    assert float(ent.min()) < 0.15, float(ent.min())
    assert float(ent.max()) < 0.85, float(ent.max())
    # GELU inputs out to about +-4 (and not orders of magnitude beyond)
    gin = torch.cat([x.flatten() for x in trace["gelu_in"]]).abs()
    assert float(torch.quantile(gin, 0.99)) >= 3.0 and float(gin.max()) <= 40.0, (float(torch.quantile(gin, 0.99)), float(gin.max()))


def test_token_classifier_argmaxes_are_clear():
    from transformers import BertConfig, BertForTokenClassification
    cfg = BertConfig(vocab_size=VOCAB, hidden_size=H, num_hidden_layers=2, num_attention_heads=12, intermediate_size=4 * H,
                     max_position_embeddings=512, num_labels=9)
    torch.manual_seed(0)
    m = BertForTokenClassification(cfg).double().eval()
    m.set_attn_implementation("eager")
    roughen(m, 3, "trained")
    bert, clf = encoder_of(m)
    assert clf is m.classifier and float(clf.bias.abs().max()) > 0
    with torch.no_grad():
        logits = m(input_ids=torch.tensor([SEQS[2]])).logits[0]
    top2 = logits.topk(2, -1).values
    assert float(((top2[:, 0] - top2[:, 1]) > 0.1).double().mean()) >= 0.8
    assert len(set(logits.argmax(-1).tolist())) >= 3                     # not one label everywhere


def _mutations(m):
    """name -> a mutated float64 copy of m (a parameter group at its default-init value, or LayerNorms mixed up)"""
    def reset(fn):
        c = copy.deepcopy(m)
        with torch.no_grad():
            fn(c)
        return c

    def each(c, fn):
        for l in c.encoder.layer:
            fn(l)
    out = {
        "b_q": lambda c: each(c, lambda l: l.attention.self.query.bias.zero_()),
        "b_k": lambda c: each(c, lambda l: l.attention.self.key.bias.zero_()),
        "b_v": lambda c: each(c, lambda l: l.attention.self.value.bias.zero_()),
        "v_takes_b_q": lambda c: each(c, lambda l: l.attention.self.value.bias.copy_(l.attention.self.query.bias)),
        "b_ao": lambda c: each(c, lambda l: l.attention.output.dense.bias.zero_()),
        "b_up": lambda c: each(c, lambda l: l.intermediate.dense.bias.zero_()),
        "b_down": lambda c: each(c, lambda l: l.output.dense.bias.zero_()),
        "ln1_g": lambda c: each(c, lambda l: l.attention.output.LayerNorm.weight.fill_(1)),
        "ln1_b": lambda c: each(c, lambda l: l.attention.output.LayerNorm.bias.zero_()),
        "ln2_g": lambda c: each(c, lambda l: l.output.LayerNorm.weight.fill_(1)),
        "ln2_b": lambda c: each(c, lambda l: l.output.LayerNorm.bias.zero_()),
        "emb_ln_g": lambda c: c.embeddings.LayerNorm.weight.fill_(1),
        "emb_ln_b": lambda c: c.embeddings.LayerNorm.bias.zero_(),
        "type_emb0": lambda c: c.embeddings.token_type_embeddings.weight[0].zero_(),
    }

    def swap(c):
        for l in c.encoder.layer:
            a, o = l.attention.output.LayerNorm, l.output.LayerNorm
            for pa, po in ((a.weight, o.weight), (a.bias, o.bias)):
                t = pa.clone()
                pa.copy_(po)
                po.copy_(t)

    def layer0(c):
        a0, o0 = c.encoder.layer[0].attention.output.LayerNorm, c.encoder.layer[0].output.LayerNorm
        for l in c.encoder.layer[1:]:
            for dst, src in ((l.attention.output.LayerNorm, a0), (l.output.LayerNorm, o0)):
                dst.weight.copy_(src.weight)
                dst.bias.copy_(src.bias)
    out["ln1<->ln2"] = swap
    out["layer0_lns"] = layer0
    return {name: reset(fn) for name, fn in out.items()}


def test_every_listed_mistake_moves_the_embedding_by_1e_3(model):
    profile, m = model
    base = [_embed_hf(m, ids) for ids in SEQS]
    moved = {}
    for name, c in _mutations(m).items():
        moved[name] = min(float((_embed_hf(c, ids) - b).abs().max()) for ids, b in zip(SEQS, base))
    P = _params(m)
    moved["fold_g_wrong_axis"] = min(float((_unit_mean(_forward(P, ids, wrong_axis=True)) - b).abs().max()) for ids, b in zip(SEQS, base))
    print(profile, " ".join(f"{k}={v:.1e}" for k, v in moved.items()))
    # a bias on K adds q . b_k to every key's logit of a query alike: the softmax cancels it exactly, so no forward - and no
    # test - can tell b_k (or K given another row's bias) from 0. Pinned as that identity rather than listed as a blind spot.
    assert moved.pop("b_k") <= 1e-12
    weak = {k: v for k, v in moved.items() if not v >= MOVE}
    assert not weak, (profile, weak)
