"""The hand-written encoders on trained-like weights (tests/encoder_weights.py) against a float64 forward.

The older encoder tests run transformers' default init: zero biases, identity LayerNorms, nearly uniform softmaxes. Under it
the LayerNorm folds of csrc/encoder_small.hpp / encoder_big.hpp reduce to the identity and the attention kernels never see a
peaked softmax. Here every module is roughened FIRST (the SmallEncoder handle copies weights and folds biases / LayerNorms at
creation), under both profiles ("trained", and "offset": pre-norm rows with |mean| / std >= 2, the fold's stress case), and
every output is compared with the same module in float64 on the CPU with eager attention - an independent high-precision
restatement. The framework's fp32 forward on the GPU is measured against the same float64 reference as the yardstick e_fw.

Bounds (raw pooled rows and hidden rows relative to the row's max |.|):
  fp32 arithmetic: within max(3 e_fw, 5e-7) - e_fw: the fp32 framework's own error - and within 1e-5 on unit rows, 2e-5 on
  raw / hidden rows (where the framework itself reaches 2.6e-5 on these weights; the kernel measured 1.1e-5);
  bf16x3 (split-bf16, three bf16 products per fp32 one; the dropped x_lo W_lo term is 2^-16 relative per GEMM): measured on these
  weights at up to 1.6e-5 on unit rows and 2.8e-4 on raw / hidden rows, with the LayerNorm folded (the small-input encoder) or
  not (the packed forward) alike - bounded at 3e-5 and 5e-4. Under default init the same arithmetic sits ~1e-6 off.
encode_many's rows equal encode's bit for bit; the NER heads' labels equal the float64 argmax wherever its top-2 logit margin
exceeds 1e-3, probabilities within 5e-5 (fp32) / 5e-4 (bf16x3). Every case prints its measured max |delta| (run with -s).
"""
import copy

import numpy as np
import pytest
import torch

from encoder_weights import PROFILES, encoder_of, roughen

pytestmark = pytest.mark.gpu

TOL = {"fp32": {"unit": 1e-5, "raw": 2e-5, "hidden": 2e-5}, "bf16x3": {"unit": 3e-5, "raw": 5e-4, "hidden": 5e-4}}
FP32_FLOOR = 5e-7
NER_PROB_TOL = {"fp32": 5e-5, "bf16x3": 5e-4}
VOCAB = 3000
ARITHS = ("fp32", "bf16x3")

# name -> (config class, config arguments). Layers: 2-4, distinct per layer. (FFN widths other than 4 x hidden: refused, below.)
MODELS = {
    "bert768": ("BertConfig", dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=3)),
    "xlmr1024": ("XLMRobertaConfig", dict(hidden_size=1024, num_attention_heads=16, intermediate_size=4096, num_hidden_layers=2,
                                          max_position_embeddings=514, pad_token_id=1, type_vocab_size=1)),
    "roberta768": ("RobertaConfig", dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=4,
                                               max_position_embeddings=514, pad_token_id=1)),
}

# one-launch form (encoder_small.hpp): every token bucket's edges, up to one 512-token sequence; packs of up to 64 sequences / 512 tokens
SMALL_CASES = [[1], [2], [15], [16], [17], [31], [32], [33], [63], [64], [65], [127], [128], [129], [256], [512],
               [5, 9, 12, 30], [17, 1, 40, 2, 23], [100, 28, 3], [8] * 64, [1] * 64, [400, 100, 12], [200, 150, 100, 62]]


def _build(name, profile, seed, layers=None, **over):
    """-> (fp32 module on the GPU, float64 module on the CPU with eager attention), the same roughened weights"""
    import transformers
    cls_name, kw = MODELS[name]
    kw = dict(kw, vocab_size=VOCAB)
    kw.setdefault("max_position_embeddings", 512)
    if layers:
        kw["num_hidden_layers"] = layers
    kw.update(over)
    cfg = getattr(transformers, cls_name)(**kw)
    model_cls = getattr(transformers, cls_name.replace("Config", "Model"))
    torch.manual_seed(0)
    m = model_cls(cfg, add_pooling_layer=False).eval()
    roughen(m, seed, profile)
    ref = copy.deepcopy(m).double()
    ref.set_attn_implementation("eager")
    return m.cuda(), ref


class _Reference:
    """float64 last hidden states per sequence (cached), and the framework's fp32 GPU forward of a padded batch"""

    def __init__(self, gpu, ref):
        self.gpu, self.ref = gpu, ref
        self.roberta = type(ref).__name__ != "BertModel"
        self.pad = int(ref.config.pad_token_id or 0)
        self.cache = {}

    def ids(self, lengths, rng):
        lo = 3 if self.roberta else 5                                   # (never the RoBERTa family's padding_idx)
        return [[int(t) for t in rng.integers(lo, VOCAB, n)] for n in lengths]

    @torch.no_grad()
    def hidden64(self, ids):
        key = tuple(ids)
        if key not in self.cache:
            self.cache[key] = self.ref(input_ids=torch.tensor([ids])).last_hidden_state[0].numpy()
        return self.cache[key]

    @torch.no_grad()
    def hidden_fw(self, seqs):
        width = max(len(x) for x in seqs)
        tok = torch.full((len(seqs), width), self.pad, dtype=torch.long)
        mask = torch.zeros((len(seqs), width), dtype=torch.long)
        for r, x in enumerate(seqs):
            tok[r, :len(x)] = torch.tensor(x)
            mask[r, :len(x)] = 1
        h = self.gpu(input_ids=tok.cuda(), attention_mask=mask.cuda()).last_hidden_state.double().cpu().numpy()
        return [h[r, :len(x)] for r, x in enumerate(seqs)]


def _pool(hiddens, pooling):
    raw = np.stack([h[0] if pooling == "cls" else h.mean(0) for h in hiddens])
    return raw, raw / np.linalg.norm(raw, axis=1, keepdims=True)


def _rel(got, want):
    """max over rows of max |delta| / max |want row|"""
    got = np.asarray(got, dtype=np.float64)
    return float(np.max(np.abs(got - want).max(1) / np.abs(want).max(1)))


class _Errors:
    """max |delta| per kind (unit pooled, raw pooled relative, hidden relative) for a kernel and for the framework"""

    def __init__(self):
        self.k = {"unit": 0.0, "raw": 0.0, "hidden": 0.0}
        self.fw = {"unit": 0.0, "raw": 0.0, "hidden": 0.0}

    def add(self, which, kind, value):
        d = self.k if which == "k" else self.fw
        d[kind] = max(d[kind], value)

    def line(self):
        return (" ".join(f"{kk} {self.k[kk]:.2e}" for kk in self.k) + " | e_fw " + " ".join(f"{kk} {self.fw[kk]:.2e}" for kk in self.fw))

    def failures(self, arith):
        bad = []
        for kind, e in self.k.items():
            if not e <= TOL[arith][kind]:
                bad.append(f"{kind} {e:.2e} > {TOL[arith][kind]:.0e}")
            if arith == "fp32" and kind in self.fw and not e <= max(3 * self.fw[kind], FP32_FLOOR):
                bad.append(f"{kind} {e:.2e} > max(3 e_fw = {3 * self.fw[kind]:.2e}, {FP32_FLOOR:.0e})")
        return bad


def _check_small(ref, encs, cases, rng, label):
    """encode (the one-launch form) over `cases`, every arithmetic, mean / CLS, unit / raw, hidden rows -> per-arithmetic failures"""
    errs = {a: _Errors() for a in encs}
    fw = _Errors()
    for lengths in cases:
        seqs = ref.ids(lengths, rng)
        want_h = [ref.hidden64(s) for s in seqs]
        fw_h = ref.hidden_fw(seqs)
        fw.add("fw", "hidden", _rel(np.concatenate(fw_h), np.concatenate(want_h)))
        for pooling in ("mean", "cls"):
            want_raw, want_unit = _pool(want_h, pooling)
            fw_raw, fw_unit = _pool(fw_h, pooling)
            fw.add("fw", "unit", float(np.abs(fw_unit - want_unit).max()))
            fw.add("fw", "raw", _rel(fw_raw, want_raw))
            for arith, enc in encs.items():
                assert enc.fits(lengths)
                unit, hid = enc.encode(seqs, pooling=pooling, normalize=True, hidden=True)
                raw = enc.encode(seqs, pooling=pooling, normalize=False)
                errs[arith].add("k", "unit", float(np.abs(unit.astype(np.float64) - want_unit).max()))
                errs[arith].add("k", "raw", _rel(raw, want_raw))
                errs[arith].add("k", "hidden", _rel(hid.cpu().numpy(), np.concatenate(want_h)))
    bad = {}
    for arith, e in errs.items():
        e.fw = fw.fw
        print(f"{label} {arith:6s} encode: {e.line()}")
        if e.failures(arith):
            bad[arith] = e.failures(arith)
    return bad


@pytest.fixture(scope="module", params=[(m, p) for m in MODELS for p in PROFILES], ids=lambda x: f"{x[0]}-{x[1]}")
def setup(request):
    from rag_project_icd10_amd import _native
    name, profile = request.param
    gpu, ref64 = _build(name, profile, seed=10 * list(MODELS).index(name) + PROFILES.index(profile))
    assert _native.SmallEncoder.supported(gpu), name
    encs = {a: _native.SmallEncoder(gpu, arithmetic=a) for a in ARITHS}   # (built after roughen: the handle folds what it sees)
    yield name, profile, gpu, _Reference(gpu, ref64), encs
    for e in encs.values():
        e.close()


def test_small_encoder_matches_float64(setup):
    name, profile, gpu, ref, encs = setup
    bad = _check_small(ref, encs, SMALL_CASES, np.random.default_rng(1), f"{name} {profile}")
    assert not bad, (name, profile, bad)


def test_encode_many_matches_encode_and_float64(setup):
    """the batch form (encoder_big.hpp) over two passes of tokens (> ENC_BIG_TMAX = 8192): every row equals the one-string call's
    bit for bit, and sampled rows sit within the bounds of float64"""
    name, profile, gpu, ref, encs = setup
    rng = np.random.default_rng(2)
    lengths = [int(n) for n in rng.integers(10, 61, 300)] + [1, 2, 129, 512]
    assert sum(lengths) > 8192 + 512
    seqs = ref.ids(lengths, rng)
    sample = list(range(0, 300, 10)) + [300, 301, 302, 303]
    want_h = [ref.hidden64(seqs[i]) for i in sample]
    fw_h = [h for i in range(0, len(sample), 16) for h in ref.hidden_fw([seqs[j] for j in sample[i:i + 16]])]
    bad = {}
    for arith, enc in encs.items():
        e = _Errors()
        for pooling, normalize in (("mean", True), ("cls", True), ("mean", False)):
            many = enc.encode_many(seqs, pooling=pooling, normalize=normalize)
            for i in range(len(seqs)):
                one = enc.encode([seqs[i]], pooling=pooling, normalize=normalize)[0]
                assert np.array_equal(many[i], one), (name, profile, arith, pooling, normalize, i)
            want_raw, want_unit = _pool(want_h, pooling)
            fw_raw, fw_unit = _pool(fw_h, pooling)
            if normalize:
                e.add("k", "unit", float(np.abs(many[sample].astype(np.float64) - want_unit).max()))
                e.add("fw", "unit", float(np.abs(fw_unit - want_unit).max()))
            else:
                e.add("k", "raw", _rel(many[sample], want_raw))
                e.add("fw", "raw", _rel(fw_raw, want_raw))
        print(f"{name} {profile} {arith:6s} encode_many: {e.line()}")
        if e.failures(arith):
            bad[arith] = e.failures(arith)
    assert not bad, (name, profile, bad)


def test_packed_split_bf16_forward_matches_float64(setup):
    """services/embedding_service.py _PackedBert (split-bf16 GEMMs with the bias rows b_hi; b_lo; the LayerNorms unfolded):
    hidden states and pooled rows, with the native packed attention and with SDPA"""
    from rag_project_icd10_amd.services.embedding_service import _PackedBert
    name, profile, gpu, ref, encs = setup
    rng = np.random.default_rng(3)
    lengths = sorted([1, 2, 17, 33, 64, 129, 300, 512] + [int(n) for n in rng.integers(3, 90, 40)], reverse=True)
    seqs = ref.ids(lengths, rng)
    want_h = [ref.hidden64(s) for s in seqs]
    pb = _PackedBert(gpu)
    native = pb.native_attention
    assert native is not None
    for use_native in (True, False):
        pb.native_attention = native if use_native else None
        hid, _ = pb.hidden_states(seqs, "cuda")
        assert pb.split_gemm, "the packed forward should run split-bf16 GEMMs on the GPU"
        e = _Errors()
        e.add("k", "hidden", _rel(hid.double().cpu().numpy(), np.concatenate(want_h)))
        for pooling in ("mean", "cls"):
            raw = pb.forward(seqs, "cuda", pooling).double().cpu().numpy()
            want_raw, want_unit = _pool(want_h, pooling)
            e.add("k", "raw", _rel(raw, want_raw))
            e.add("k", "unit", float(np.abs(raw / np.linalg.norm(raw, axis=1, keepdims=True) - want_unit).max()))
        print(f"{name} {profile} packed native_attention={use_native}: {e.line()}")
        assert not e.failures("bf16x3"), (name, profile, use_native, e.failures("bf16x3"))   # (split-bf16 GEMMs: that arithmetic's bounds)


@pytest.mark.parametrize("profile", PROFILES)
def test_twelve_layers_on_short_strings(profile):
    from rag_project_icd10_amd import _native
    gpu, ref64 = _build("bert768", profile, seed=12, layers=12)
    encs = {a: _native.SmallEncoder(gpu, arithmetic=a) for a in ARITHS}
    try:
        cases = [[1], [2], [5], [9], [16], [23], [3, 11, 7, 20, 14]]
        bad = _check_small(_Reference(gpu, ref64), encs, cases, np.random.default_rng(4), f"bert768x12 {profile}")
        assert not bad, (profile, bad)
    finally:
        for e in encs.values():
            e.close()


@pytest.mark.parametrize("profile", PROFILES)
def test_ner_small_and_packed_paths_match_float64(profile):
    """MedicalNERService's token classifier (services/medical_ner_service.py _TokenClassifier): the small-input path (one launch
    of encoder_small.hpp, <= 64 strings and 512 tokens) and the packed split-bf16 path (> 32 strings that do not fit one call),
    roughened encoder AND classifier, against the float64 logits"""
    from transformers import BertConfig, BertForTokenClassification
    from rag_project_icd10_amd.services.medical_ner_service import _CharOffsetTokenizer, _TokenClassifier
    labels = ["O"] + [f"{p}-T{i}" for i in range(4) for p in ("B", "I")]
    cfg = BertConfig(vocab_size=VOCAB, hidden_size=768, num_attention_heads=12, intermediate_size=3072, num_hidden_layers=3,
                     max_position_embeddings=512, num_labels=len(labels), id2label=dict(enumerate(labels)),
                     label2id={l: i for i, l in enumerate(labels)})
    torch.manual_seed(0)
    model = BertForTokenClassification(cfg).eval()
    roughen(model, 21, profile)
    ref = copy.deepcopy(model).double()
    ref.set_attn_implementation("eager")
    clf = _TokenClassifier(model, _CharOffsetTokenizer(VOCAB, 512), cfg.id2label, "cuda")
    assert clf._small is not None and clf._packed is not None
    rng = np.random.default_rng(5)

    def seq(n):
        return [101] + [int(t) for t in rng.integers(1000, VOCAB, n - 2)] + [102]
    small_groups = [[seq(2)], [seq(n) for n in (9, 30, 17)], [seq(n) for n in rng.integers(3, 20, 40)], [seq(200), seq(300)]]
    packed = [seq(int(n)) for n in rng.integers(5, 40, 80)] + [seq(400)]
    from rag_project_icd10_amd import _native
    small_fp32 = _native.SmallEncoder(encoder_of(clf.model)[0], arithmetic="fp32")
    small_default = clf._small                                     # (the service's arithmetic, bf16x3 by default)
    runs = ([("small", small_default.arithmetic, g) for g in small_groups] + [("small", "fp32", g) for g in small_groups]
            + [("packed", "bf16x3", packed)])
    worst, clear, total = {}, 0, 0
    try:
        for path, arith, group in runs:
            clf._small = small_fp32 if (path, arith) == ("small", "fp32") else small_default
            lengths = [len(s) for s in group]
            assert clf._small.fits(lengths) == (path == "small") and (path == "small" or len(group) > 32)
            got = clf._forward([(s, None, None, None) for s in group])
            for s, (lab, prob) in zip(group, got):
                with torch.no_grad():
                    logits = ref(input_ids=torch.tensor([s])).logits[0]
                top2 = logits.topk(2, -1).values
                sure = (top2[:, 0] - top2[:, 1]).numpy() > 1e-3
                want = logits.argmax(-1).numpy()
                assert np.array_equal(np.asarray(lab)[sure], want[sure]), (profile, path, arith, len(s))
                d = float(np.abs(np.asarray(prob, dtype=np.float64) - torch.softmax(logits, -1).max(-1).values.numpy()).max())
                worst[(path, arith)] = max(worst.get((path, arith), 0.0), d)
                clear += int(sure.sum())
                total += len(s)
    finally:
        clf._small = small_default
        small_fp32.close()
    print(f"ner {profile}: max |d probability| " + ", ".join(f"{p} {a} {v:.2e}" for (p, a), v in worst.items())
          + f"; {clear} of {total} tokens with a float64 margin > 1e-3")
    for (path, arith), v in worst.items():
        assert v <= NER_PROB_TOL[arith], (profile, path, arith, v)
    assert clear >= 0.95 * total


@pytest.mark.parametrize("inter", [1536, 2304])
def test_ffn_widths_other_than_four_times_hidden_are_refused(inter):
    """icd_encoder_create's FFN-down GEMM covers its outputs with exactly four waves (inter = 4 x hidden): narrower FFNs, which
    it once admitted and then left outputs unwritten for, are refused - by supported() (the services keep the framework's
    forward then) and by the library itself"""
    from rag_project_icd10_amd import _native
    gpu, _ = _build("bert768", "trained", seed=1, layers=2, intermediate_size=inter)
    assert not _native.SmallEncoder.supported(gpu)
    with pytest.raises(_native.IcdError, match="inter"):
        _native.SmallEncoder(gpu)
