"""Inputs shared by tests/test_semantic_cpu.py and tests/test_semantic_gpu.py: the catalogue of the semantic-fit tests."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

FILMS = ["star wars", "the empire strikes back", "return of the jedi", "alien", "aliens", "blade runner", "the matrix", "matrix reloaded", "dune"]


def tiny_words():
    """whole words of the tiny tokenizer's vocabulary (no specials, no continuation pieces, no single characters)"""
    vocab = json.load(open(os.path.join(GOLDEN, "tokenizer_tiny.json"), encoding="utf-8"))["model"]["vocab"]
    return sorted(w for w in vocab if len(w) > 1 and w.isascii() and w.isalpha())


def catalogue():
    """150 texts of 0 ... 30 words with a fixed seed: 2 tokens ([CLS] [SEP]) up to the truncation length of 24; row 5 is the empty
    string, row 70 has 30 words (longer than max_length), row 149 a single word"""
    rng = np.random.default_rng(16)
    words = tiny_words()
    texts = [" ".join(rng.choice(words, size=int(rng.integers(0, 31)))) for _ in range(150)]
    texts[5] = ""
    texts[70] = " ".join(rng.choice(words, size=30))
    texts[149] = words[3]
    return [f"item-{i}" for i in range(150)], texts
