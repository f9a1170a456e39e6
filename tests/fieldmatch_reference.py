"""The reference's term / ngram / BM25 field matchers, transcribed line by line (no GPU, no library): what the tests of the
device-matched field_match columns compare with.

    feature/matcher/FieldMatcher.scala:15-65   score (merge walk), unique
    feature/matcher/NgramMatcher.scala:10-30   tokenize
    feature/matcher/BM25Matcher.scala:20-40    score
    feature/FieldMatchFeature.scala:60-92      values: which items get 0

Strings are compared as java.lang.String.compareTo does: by UTF-16 code unit, then by length.  math.log stands in for the
JVM's Math.log (DESIGN.md lists it with the other unpinned items).
"""
import math

K1 = 1.2   # as in Lucene
B = 0.75   # as in Lucene


def utf16_key(s: str):
    """the UTF-16 code units of s: tuples of them order like String.compareTo"""
    b = s.encode("utf-16-be", "surrogatepass")
    return tuple((b[i] << 8) | b[i + 1] for i in range(0, len(b), 2))


def compare_to(a: str, b: str) -> int:
    ka, kb = utf16_key(a), utf16_key(b)
    return -1 if ka < kb else (1 if ka > kb else 0)


def strictly_ascending(tokens) -> bool:
    return all(compare_to(tokens[i - 1], tokens[i]) < 0 for i in range(1, len(tokens)))


def unique(buffer):
    """FieldMatcher.unique: Arrays.sort(naturalOrder) + in-place dedup"""
    buffer = sorted(buffer, key=utf16_key)
    if not buffer:
        return buffer
    pos = 0
    i = 1
    while i < len(buffer):
        if buffer[pos] == buffer[i]:
            i += 1
        else:
            pos += 1
            buffer[pos] = buffer[i]
            i += 1
    return buffer if pos + 1 == i else buffer[:pos + 1]


def term_tokenize(terms):
    """TermMatcher.tokenize after language.split (the analyzers stay on the JVM: `terms` is their output)"""
    return [] if len(terms) == 0 else unique(list(terms))


def ngram_tokenize(terms, n: int):
    """NgramMatcher.tokenize after language.split; substring works on UTF-16 code units"""
    if len(terms) == 0:
        return []
    buf = []
    i = 0
    while i < len(terms):
        units = utf16_key(terms[i])
        j = 0
        while j <= len(units) - n:
            gram = units[j:j + n]
            buf.append(b"".join(u.to_bytes(2, "big") for u in gram).decode("utf-16-be", "surrogatepass"))
            j += 1
        i += 1
    return unique(buf)


def match_score(query, doc) -> float:
    """FieldMatcher.score: the merge walk itself, not set arithmetic"""
    if len(query) == 0 or len(doc) == 0:
        return 0.0
    i = 0
    j = 0
    union = 0
    intersection = 0
    while i < len(query) or j < len(doc):
        if i < len(query) and j < len(doc):
            if compare_to(query[i], doc[j]) == 0:
                intersection += 1
                union += 1
                i += 1
                j += 1
            elif compare_to(query[i], doc[j]) < 0:
                union += 1
                i += 1
            else:
                union += 1
                j += 1
        else:
            if i < len(query):
                union += 1
                i += 1
            else:
                union += 1
                j += 1
    return float(intersection) / float(union)


def _int32(v: int) -> int:
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def bm25_idf(docs: int, gtf: int) -> float:
    return math.log(1.0 + (_int32(docs - gtf) + 0.5) / (gtf + 0.5))


def bm25_score(query, doc, dic) -> float:
    """BM25Matcher.score; dic = {"docs", "avgdl", "termfreq"}.  Python floats are IEEE doubles and every operator rounds once,
    as the JVM's do."""
    total = 0.0
    i = 0
    doc_freq = {}
    for t in doc:
        doc_freq[t] = doc_freq.get(t, 0) + 1
    while i < len(query):
        term = query[i]
        doc_term_freq = doc_freq.get(term, 0)
        global_term_freq = dic["termfreq"].get(term, 0)
        term_idf = bm25_idf(dic["docs"], global_term_freq)
        total += term_idf * (doc_term_freq * (K1 + 1.0)) / (doc_term_freq + K1 * (1.0 - B + B * (len(doc) / dic["avgdl"])))
        i += 1
    return total


def column(method: str, query, states, dic=None):
    """FieldMatchFeature.values for one request: `query` = the request's tokens or None (field absent); `states` = per item the
    stored token list, or None for an unknown item / no state / state of another type."""
    out = []
    for doc in states:
        if query is None or doc is None:
            out.append(0.0)
        elif method == "bm25":
            out.append(bm25_score(query, doc, dic))
        else:
            out.append(match_score(query, doc))
    return out
