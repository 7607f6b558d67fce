"""Seeded byte-level BPE tokenizer.json files for the BPE tests (trained offline with `tokenizers`; nothing is downloaded), and
`spec_ids`: a pure-Python restatement of what csrc/bpe.hip does -- the NFC proof, the greedy cut of space runs, the local
pre-token rule and lowest-rank-first merging.  The oracle of both is HF `tokenizers` built from the same file."""
import json
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_bpe_table as table  # noqa: E402

SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
VARIANTS = {
    "nfc_runs": dict(nfc=True, runs=tuple(range(2, 25))),
    "nfc_plain": dict(nfc=True, runs=()),
    "raw_runs48": dict(nfc=False, runs=(4, 8)),
    "ignore_merges": dict(nfc=True, runs=tuple(range(2, 25)), ignore_merges=True),
}
_WORDS = ["the", "quick", "brown", "fox", "hello", "world", "token", "tokenizer", "tokenization", "it's", "don't", "we're", "I've", "I'm",
          "they'll", "he'd", "café", "naïve", "résumé", "straße", "привет", "мир", "中文", "東京", "x=1", "a,b", "2024", "3.14", "foo_bar", "()",
          "...", "!!", "=====", "--", "that's", "can't", "é", "한국어"]
_cache = {}


def corpus(seed=0, n=3000):
    rng = random.Random(seed)
    letters = "abcdefghijklmnopqrstuvwxyz"
    words = list(_WORDS) + ["".join(rng.choice(letters) for _ in range(rng.randint(2, 8))) for _ in range(300)]
    seps = [" "] * 8 + ["  ", "\n", "\t", ", ", ". ", "   ", " \n", "\n\n"]
    return ["".join(rng.choice(words) + rng.choice(seps) for _ in range(rng.randint(1, 12))) for _ in range(n)]


def tokenizer_json(nfc=True, runs=(), ignore_merges=False, vocab_size=1200, seed=0) -> str:
    key = (nfc, tuple(runs), ignore_merges, vocab_size, seed)
    if key in _cache:
        return _cache[key]
    from tokenizers import AddedToken, Tokenizer, models, normalizers, pre_tokenizers, processors, trainers

    tok = Tokenizer(models.BPE())
    if nfc:
        tok.normalizer = normalizers.NFC()
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=list(SPECIALS), initial_alphabet=pre_tokenizers.ByteLevel.alphabet(),
                                  show_progress=False)
    tok.train_from_iterator(corpus(seed), trainer)
    if runs:
        tok.add_tokens([AddedToken(" " * n, normalized=True, lstrip=False, rstrip=False, single_word=False) for n in runs])
    cls_id, sep_id = tok.token_to_id("[CLS]"), tok.token_to_id("[SEP]")
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
                                                       special_tokens=[("[CLS]", cls_id), ("[SEP]", sep_id)])
    spec = json.loads(tok.to_str())
    spec["model"]["ignore_merges"] = bool(ignore_merges)
    _cache[key] = json.dumps(spec, ensure_ascii=False)
    return _cache[key]


def write_tokenizer(path, **kw) -> str:
    with open(path, "w", encoding="utf-8") as f:
        f.write(tokenizer_json(**kw))
    return str(path)


# ------------------------------------------------------------------------------------------ the kernel's specification
def greedy_tables(space_ids):
    """(M, lg, cons) as vrag_bpe_create builds them: lg[x] = the largest run token <= x, cons[x] = spaces of x < M consumed."""
    lg, m = [], 0
    for n, i in enumerate(space_ids):
        if i >= 0:
            m = n
        lg.append(m)
    cons = []
    for x in range(max(m, 1)):
        rem = x
        while lg[rem]:
            rem -= lg[rem]
        cons.append(x - rem)
    return m, lg, cons


def spec_pieces(text, cfg):
    """[(piece, length of the space-run token or 0)] of `text`, or None when the device would flag it."""
    import unicodedata

    n = len(text)
    cps = [ord(ch) for ch in text]
    cls = []
    for i, c in enumerate(cps):
        if not table.covered(c):
            return None
        if cfg["nfc"]:
            if not table.nfc_qc_yes(c):
                return None
            ccc = unicodedata.combining(text[i])
            if ccc and i and unicodedata.combining(text[i - 1]) > ccc:
                return None
        cls.append(table.char_class(c))
    L, N, W = table.L, table.N, table.W
    NONE, SPACE = 4, 5
    M, lg, cons = greedy_tables(cfg["space_ids"])

    def consumed(r):
        return (r // M) * M + cons[r % M] if M else 0

    def token_at(r, k):
        q = (r // M) * M
        if k < q:
            return M if k % M == 0 else 0
        pos = q
        while True:
            t = lg[r - pos]
            if k == pos:
                return t
            if k < pos + t:
                return 0
            pos += t

    def run_of(i):      # (start, length) of the run of U+0020 around i
        a = i
        while a and cps[a - 1] == 0x20:
            a -= 1
        b = i
        while b + 1 < n and cps[b + 1] == 0x20:
            b += 1
        return a, b - a + 1

    def prev_kind(i):
        if i == 0:
            return NONE
        if cps[i - 1] != 0x20:
            return cls[i - 1]
        _a, r = run_of(i - 1)
        return NONE if consumed(r) == r else SPACE

    def contraction_at(j):
        tail = text[j + 1:j + 3]
        k = 2 if tail[:1] in ("s", "t", "m", "d") else 3 if tail in ("re", "ve", "ll") else 0
        return k if k and prev_kind(j) in (NONE, L, N, W) else 0

    def contraction_state(i):
        if i >= 1 and text[i - 1] == "'" and contraction_at(i - 1):
            return 1
        if i >= 2 and text[i - 2] == "'":
            k = contraction_at(i - 2)
            if k:
                return 1 if k == 3 else 2
        if i >= 3 and text[i - 3] == "'" and contraction_at(i - 3) == 3:
            return 2
        return 0

    starts = []      # (index, space-run token length)
    for i, c in enumerate(cps):
        if c == 0x20:
            a, r = run_of(i)
            k, used = i - a, consumed(r)
            if k < used:
                t = token_at(r, k)
                if t:
                    starts.append((i, t))
                continue
            prev_ws = True if k > used else False if k > 0 else (i > 0 and cls[i - 1] == W)
            next_text = k == r - 1 and i + 1 < n and cls[i + 1] != W
            start = not prev_ws or next_text
        else:
            pk = prev_kind(i)
            if cls[i] == W:
                next_text = i + 1 < n and cps[i + 1] != 0x20 and cls[i + 1] != W
                start = pk not in (SPACE, W) or next_text
            else:
                cs = contraction_state(i) if cls[i] == L else 0
                start = False if cs == 1 else True if cs == 2 else pk not in (cls[i], SPACE)
        if start:
            starts.append((i, 0))
    assert not text or starts[0][0] == 0
    out = []
    for (i, t), nxt in zip(starts, [s for s, _t in starts[1:]] + [n]):
        assert not t or nxt - i == t
        out.append((text[i:nxt], t))
    return out


def spec_ids(text, cfg):
    """The ids of `text` without special tokens, or None when the device would flag it (a pre-token beyond the cap included)."""
    pieces = spec_pieces(text, cfg)
    if pieces is None:
        return None
    left, right, merged = cfg["merges"]
    rank = {(a, b): (r, m) for r, (a, b, m) in enumerate(zip(left, right, merged))}
    whole = dict(cfg["whole"])
    ids = []
    for piece, run in pieces:
        if run:
            ids.append(cfg["space_ids"][run])
            continue
        raw = piece.encode("utf-8")
        if len(raw) > 64:
            return None
        if cfg["ignore_merges"] and raw in whole:
            ids.append(whole[raw])
            continue
        sym = [cfg["byte_ids"][b] for b in raw]
        while len(sym) > 1:
            best = min(((rank[p][0], k) for k, p in enumerate(zip(sym, sym[1:])) if p in rank), default=None)
            if best is None:
                break
            k = best[1]
            sym[k:k + 2] = [rank[(sym[k], sym[k + 1])][1]]
        ids.extend(sym)
    return ids
