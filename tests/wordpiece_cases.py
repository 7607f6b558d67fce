"""Seeded BERT-style vocabularies and tokenizer.json files for the WordPiece tests; the oracle is HF `tokenizers` built from
the same file.  Nothing is downloaded."""
import json
import random
import string

SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
CJK = "中文字漢語日本東京大学你好世界人山水火木金土"


def make_vocab(seed: int = 0, n_words: int = 400, size: int = 0):
    """About 2k pieces: every ASCII letter / digit / punctuation mark alone and as a ## piece, multi-character words and
    suffixes, CJK ideographs, accent-stripped / lowercased and accented / cased forms.  `size`: padded with [unusedN] up to it."""
    rng = random.Random(seed)
    pieces = list(SPECIALS)
    seen = set(pieces)

    def add(p):
        if p not in seen:
            seen.add(p)
            pieces.append(p)

    for ch in string.ascii_letters + string.digits + string.punctuation:
        add(ch)
        add("##" + ch)
    for w in ("un", "una", "unaff", "##aff", "##able", "##ffable", "##a", "able", "affable", "the", "quick", "brown", "fox", "##s", "##ing",
              "##ed", "token", "##izer", "##ization", "hello", "world", "resume", "cafe", "café", "résumé", "Hello", "World", "naive", "naïve",
              "straße", "strasse", "αβγ", "привет", "мир", "##ет", "ab", "##b", "a", "##c"):
        add(w)
    letters = string.ascii_lowercase
    while len(pieces) < 5 + 2 * 94 + 40 + n_words:
        w = "".join(rng.choice(letters) for _ in range(rng.randint(2, 9)))
        add(w if rng.random() < 0.6 else "##" + w)
        if rng.random() < 0.2:
            add(w.capitalize())
    for ch in CJK:
        add(ch)
        add("##" + ch)
    for ch in "éèüöñçåøßæœ":
        add(ch)
        add("##" + ch)
    i = 0
    while len(pieces) < size:
        add(f"[unused{i}]")
        i += 1
    return pieces


def tokenizer_spec(pieces, lowercase=True, strip_accents=None, clean_text=True, handle_chinese_chars=True):
    vocab = {p: i for i, p in enumerate(pieces)}
    cls_id, sep_id = vocab["[CLS]"], vocab["[SEP]"]
    return {
        "version": "1.0", "truncation": None, "padding": None,
        "added_tokens": [{"id": vocab[t], "content": t, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False,
                          "special": True} for t in SPECIALS],
        "normalizer": {"type": "BertNormalizer", "clean_text": clean_text, "handle_chinese_chars": handle_chinese_chars,
                       "strip_accents": strip_accents, "lowercase": lowercase},
        "pre_tokenizer": {"type": "BertPreTokenizer"},
        "post_processor": {"type": "TemplateProcessing",
                           "single": [{"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
                                      {"SpecialToken": {"id": "[SEP]", "type_id": 0}}],
                           "pair": [{"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
                                    {"SpecialToken": {"id": "[SEP]", "type_id": 0}}, {"Sequence": {"id": "B", "type_id": 1}},
                                    {"SpecialToken": {"id": "[SEP]", "type_id": 1}}],
                           "special_tokens": {"[CLS]": {"id": "[CLS]", "ids": [cls_id], "tokens": ["[CLS]"]},
                                              "[SEP]": {"id": "[SEP]", "ids": [sep_id], "tokens": ["[SEP]"]}}},
        "decoder": {"type": "WordPiece", "prefix": "##", "cleanup": True},
        "model": {"type": "WordPiece", "unk_token": "[UNK]", "continuing_subword_prefix": "##", "max_input_chars_per_word": 100,
                  "vocab": vocab},
    }


def write_tokenizer(path, pieces, **kw):
    with open(path, "w", encoding="utf-8") as f:
        json.dump(tokenizer_spec(pieces, **kw), f, ensure_ascii=False)
    return str(path)
