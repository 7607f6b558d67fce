"""Device WordPiece tokenizer, the parts that need no GPU: which tokenizer.json files it takes, and the committed table."""
import copy
import importlib.util
import json
import os
import re
import unicodedata

import pytest

import verbatim_rag_amd  # noqa: F401
from verbatim_rag_amd import wordpiece
from wordpiece_cases import make_vocab, tokenizer_spec, write_tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_accepts_a_bert_tokenizer_json(tmp_path):
    pieces = make_vocab()
    path = write_tokenizer(tmp_path / "tokenizer.json", pieces)
    cfg = wordpiece.parse_spec(json.load(open(path, encoding="utf-8")), path)
    assert cfg["pieces"] == pieces and (cfg["unk_id"], cfg["cls_id"], cfg["sep_id"]) == (1, 2, 3)
    assert cfg["flags"] == 1 | 2 | 4 | 8 and cfg["prefix"] == "##" and cfg["max_chars"] == 100      # strip_accents null follows lowercase
    cased = wordpiece.parse_spec(tokenizer_spec(pieces, lowercase=False, strip_accents=False))
    assert cased["flags"] == 4 | 8
    assert wordpiece.parse_spec(tokenizer_spec(pieces, lowercase=False, strip_accents=None))["flags"] == 4 | 8
    assert "[SEP]" in cfg["added"] and "[MASK]" in cfg["added"]


def test_from_file_rejects_the_bpe_golden_file():
    with pytest.raises(ValueError, match="model must be WordPiece"):
        wordpiece.GpuWordPieceTokenizer.from_file(os.path.join(ROOT, "tests", "golden", "tokenizer.json"))


def _deviations():
    def model(s):
        s["model"] = {"type": "WordLevel", "vocab": s["model"]["vocab"], "unk_token": "[UNK]"}

    def normalizer(s):
        s["normalizer"] = {"type": "NFC"}

    def no_normalizer(s):
        s["normalizer"] = None

    def pre(s):
        s["pre_tokenizer"] = {"type": "Whitespace"}

    def post(s):
        s["post_processor"] = {"type": "BertProcessing", "sep": ["[SEP]", 3], "cls": ["[CLS]", 2]}

    def template(s):
        s["post_processor"]["single"] = s["post_processor"]["single"][1:]

    def added(s):
        s["added_tokens"].append({"id": 5, "content": "a", "single_word": False, "lstrip": False, "rstrip": False, "normalized": True,
                                  "special": False})

    return [("added_tokens", added), ("model", model), ("normalizer", normalizer), ("normalizer", no_normalizer), ("pre_tokenizer", pre),
            ("post_processor", post), ("post_processor", template)]


@pytest.mark.parametrize("component,change", _deviations(), ids=lambda x: x if isinstance(x, str) else x.__name__)
def test_from_file_rejects_each_single_component_deviation(tmp_path, component, change):
    spec = copy.deepcopy(tokenizer_spec(make_vocab()))
    change(spec)
    path = tmp_path / "tokenizer.json"
    path.write_text(json.dumps(spec, ensure_ascii=False), encoding="utf-8")
    with pytest.raises(ValueError, match=component):
        wordpiece.GpuWordPieceTokenizer.from_file(str(tmp_path))      # a directory works as well as the file


def test_exported_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "vrag_amd.h")).read()
    assert int(re.search(r"#define VRAG_WORDPIECE_TILE_BYTES (\d+)", hdr).group(1)) == wordpiece.TILE_BYTES
    assert int(re.search(r"#define VRAG_WP_MAX_CHARS_PER_WORD (\d+)", hdr).group(1)) == wordpiece.MAX_CHARS_PER_WORD


def test_committed_table_is_what_the_generator_produces():
    import tokenizers

    spec = importlib.util.spec_from_file_location("_gen_wp", os.path.join(ROOT, "tools", "gen_wordpiece_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    uni, tok = gen.recorded_versions()
    if uni != unicodedata.unidata_version:
        pytest.skip(f"the table records unicodedata {uni}, this interpreter has {unicodedata.unidata_version}")
    if tok != tokenizers.__version__:
        pytest.skip(f"the table records tokenizers {tok}, installed is {tokenizers.__version__}")
    with open(gen.OUT, encoding="utf-8") as f:
        assert f.read() == gen.render()
