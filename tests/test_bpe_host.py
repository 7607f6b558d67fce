"""The host side of the byte-level BPE tokenizer (verbatim_rag_amd/bpe.py, tools/gen_bpe_table.py): which tokenizer.json files
are accepted, and the kernel's specification -- `bpe_cases.spec_ids`, a pure-Python restatement of the NFC proof, the space-run
cuts, the local pre-token rule and the merge order -- against HF `tokenizers`.  Needs no GPU."""
import copy
import json
import os
import random
import subprocess
import sys

import pytest

from bpe_cases import VARIANTS, spec_ids, spec_pieces, tokenizer_json

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spec(name="nfc_runs"):
    return json.loads(tokenizer_json(**VARIANTS[name]))


@pytest.mark.parametrize("name", list(VARIANTS))
def test_parse_spec_accepts_the_variants(name):
    from verbatim_rag_amd.bpe import MAX_SPACE_RUN, parse_spec

    spec = _spec(name)
    cfg = parse_spec(spec)
    kw = VARIANTS[name]
    assert cfg["nfc"] == kw["nfc"] and cfg["ignore_merges"] == bool(kw.get("ignore_merges"))
    assert [n for n in range(MAX_SPACE_RUN + 1) if cfg["space_ids"][n] >= 0] == list(kw["runs"])
    assert sorted(cfg["routed"]) == sorted(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"])
    assert cfg["n_vocab"] == len(spec["model"]["vocab"]) + len(kw["runs"]) and (cfg["cls_id"], cfg["sep_id"]) == (2, 3)
    assert len(cfg["merges"][0]) == len(spec["model"]["merges"]) > 500 and len(set(cfg["byte_ids"])) == 256
    assert bool(cfg["whole"]) == bool(kw.get("ignore_merges"))
    as_strings = copy.deepcopy(spec)      # merges as "a b" strings, the older serialisation
    as_strings["model"]["merges"] = [m if isinstance(m, str) else " ".join(m) for m in spec["model"]["merges"]]
    assert parse_spec(as_strings)["merges"] == cfg["merges"]


def _broken(change):
    spec = _spec()
    change(spec)
    return spec


def _drop_byte(spec):
    del spec["model"]["vocab"]["\u0120"]      # the byte-level character of 0x20


def _lstrip_run(spec):
    next(t for t in spec["added_tokens"] if t["content"] == "  ")["lstrip"] = True


REFUSED = {
    "model must be BPE": lambda s: s["model"].update(type="WordPiece"),
    "add_prefix_space": lambda s: s["pre_tokenizer"].update(add_prefix_space=True),
    "use_regex": lambda s: s["pre_tokenizer"].update(use_regex=False),
    "pre_tokenizer must be ByteLevel": lambda s: s.update(pre_tokenizer={"type": "Whitespace"}),
    "dropout": lambda s: s["model"].update(dropout=0.1),
    "byte_fallback": lambda s: s["model"].update(byte_fallback=True),
    "post_processor must be TemplateProcessing": lambda s: s.update(post_processor={"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": True}),
    "byte 0x20": _drop_byte,
    "lstrip": _lstrip_run,
    "normalizer must be null or NFC": lambda s: s.update(normalizer={"type": "NFKC"}),
    "continuing_subword_prefix": lambda s: s["model"].update(continuing_subword_prefix="##"),
    "changes under NFC": lambda s: s["added_tokens"].append(dict(s["added_tokens"][-1], id=len(s["model"]["vocab"]) + 23, content="e\u0301")),
}


@pytest.mark.parametrize("message", list(REFUSED))
def test_parse_spec_refuses_naming_the_component(message):
    from verbatim_rag_amd.bpe import parse_spec

    with pytest.raises(ValueError, match=message):
        parse_spec(_broken(REFUSED[message]), "some/tokenizer.json")


def test_parse_spec_takes_dropout_zero_and_the_golden_bpe_file_is_not_byte_level():
    from verbatim_rag_amd.bpe import parse_spec

    parse_spec(_broken(lambda s: s["model"].update(dropout=0.0)))
    with open(os.path.join(ROOT, "tests", "golden", "tokenizer.json"), encoding="utf-8") as f:
        with pytest.raises(ValueError, match="normalizer|pre_tokenizer must be ByteLevel"):
            parse_spec(json.load(f))


def test_byte_alphabet_is_the_library_s():
    from tokenizers.pre_tokenizers import ByteLevel

    from verbatim_rag_amd.bpe import byte_alphabet

    mine = byte_alphabet()
    assert sorted(mine) == sorted(ByteLevel.alphabet()) and len(set(mine)) == 256
    pre = ByteLevel(add_prefix_space=False, use_regex=False)
    for b in (0x00, 0x20, 0x21, 0x7E, 0x7F, 0xA0, 0xAD, 0xFF):      # one byte at a time through latin-1 -> 2-byte UTF-8 would not do
        if b < 0x80:
            assert pre.pre_tokenize_str(chr(b))[0][0] == mine[b]
    assert pre.pre_tokenize_str("\u00ff")[0][0] == mine[0xC3] + mine[0xBF]


def _random_texts(seed, n):
    rng = random.Random(seed)
    alphabet = (["'"] * 10 + [" "] * 14 + ["\n"] * 3 + ["\t"] * 2 + list("stremvld") * 3 + list("abcxyzSTQ") + list("0123456789")
                + list(".,!?-=()\"") + ["\u00e9", "\u00df", "\u4e2d", "\u0436", "\u00a0", "\u3000", "\u0085", "\U0001F600", "\u0301", "\u0327", "\u2028"])
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, 40))) for _ in range(n)]


@pytest.mark.parametrize("name", list(VARIANTS))
def test_the_specification_equals_hf_on_random_strings(name):
    """Every id of every string the specification does not flag; and it flags little: only what fails the NFC proof."""
    from tokenizers import Tokenizer

    from verbatim_rag_amd.bpe import parse_spec

    spec = _spec(name)
    cfg = parse_spec(spec)
    hf = Tokenizer.from_str(json.dumps(spec))
    texts = _random_texts(11, 3000) + [" " * r + w for r in range(0, 60) for w in ("", "a", "'s", "\n")] + \
        ["a" + " " * r + w for r in range(0, 60) for w in ("", "b", "'ll x", "\n", "1")]
    flagged = 0
    for text, enc in zip(texts, hf.encode_batch(texts, add_special_tokens=False)):
        got = spec_ids(text, cfg)
        if got is None:
            flagged += 1
            assert cfg["nfc"] and ("\u0301" in text or "\u0327" in text), repr(text)
            continue
        assert got == list(enc.ids), (repr(text), spec_pieces(text, cfg), enc.tokens)
    assert flagged < len(texts) // 3 and (flagged > 0) == cfg["nfc"]


def test_the_specification_on_the_observed_cases():
    from verbatim_rag_amd.bpe import parse_spec

    cfg = parse_spec(_spec("nfc_runs"))

    def pieces(text):
        return [p for p, _t in spec_pieces(text, cfg)]

    assert pieces("a's") == ["a", "'s"] and pieces("a 's") == ["a", " '", "s"] and pieces("!'s") == ["!'", "s"]
    assert pieces("a\n's") == ["a", "\n", "'s"] and pieces("A'S") == ["A", "'", "S"]
    assert spec_pieces("a  's", cfg) == [("a", 0), ("  ", 2), ("'s", 0)] and spec_pieces("x  ", cfg) == [("x", 0), ("  ", 2)]
    assert [t for _p, t in spec_pieces(" " * 26, cfg)] == [24, 2]
    assert spec_pieces("e\u0301", cfg) is None and spec_pieces("\u00e9", cfg) is not None
    assert spec_pieces("a\u0301\u0327", cfg) is None      # marks of descending combining class (230, 202)
    assert spec_pieces("a\ue000", cfg) is None            # private use: not covered


def test_committed_table_is_what_the_generator_writes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_bpe_table.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


def test_bpe_kernels_keep_everything_in_registers():
    """The merge kernel hides dependent L2 gathers by occupancy, so it must stay small; none of the kernels may use scratch."""
    from test_kernel_resources import HIPCC, _resources

    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    rows = {r["name"]: r for r in _resources("bpe.hip") if "bpe_" in r["name"]}
    assert len(rows) == 4      # tile runs, bounds x 2, merge
    for name, r in rows.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0, r
        if "merge" in name:
            assert int(r["VGPRs"]) <= 64 and int(r["LDS Size [bytes/block]"]) == 0, r
