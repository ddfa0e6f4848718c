"""CPU-only: every device buffer of the context and of a verification lane is named exactly once in the list that classes it as
resident or scratch (ctx.h, for_each_buffer).  That list is what dsm_ctx_memory_footprint counts, what a smaller
dsm_ctx_set_memory_budget releases and what the verifier's out-of-memory retry gives back: a buffer missing from it is never
counted."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx_h():
    text = open(os.path.join(ROOT, "dagsfm_amd", "csrc", "ctx.h")).read()
    return re.sub(r"//[^\n]*", "", text)


def _struct_body(text, name):
    start = text.index("struct %s {" % name) + len("struct %s {" % name)
    depth, i = 1, start
    while depth:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        i += 1
    return text[start:i - 1]


def _declared_bufs(body):
    """DevBuf members declared at the top level of a struct body, arrays expanded to their elements."""
    top, depth = [], 0
    for ch in body:
        depth += ch == "{"
        if depth == 0:
            top.append(ch)
        depth -= ch == "}"
    names = []
    for decl in re.findall(r"\bDevBuf\s+([^;()]+);", "".join(top)):
        for item in decl.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", item)
            assert m, item
            names += [m.group(1)] if m.group(2) is None else ["%s[%d]" % (m.group(1), k) for k in range(int(m.group(2)))]
    return names


def _listed_bufs(body):
    """(buffer, scratch) for every &name in the for_each_buffer lists of a struct body."""
    fn = body[body.index("void for_each_buffer("):]
    out = []
    for lst, rest in re.findall(r"for \(DevBuf\* b : \{([^}]*)\}\)\s*([^;]*);", fn):
        scratch = {"f(*b)": True, "f(*b, true)": True, "f(*b, false)": False}[rest.strip()]
        out += [(n, scratch) for n in re.findall(r"&(\w+(?:\[\d+\])?)", lst)]
    return out


def _check(struct):
    body = _struct_body(_ctx_h(), struct)
    declared = _declared_bufs(body)
    listed = [n for n, _ in _listed_bufs(body)]
    assert len(declared) == len(set(declared))
    twice = sorted({n for n in listed if listed.count(n) > 1})
    assert not twice, "%s::for_each_buffer names these twice: %s" % (struct, twice)
    missing = sorted(set(declared) - set(listed))
    assert not missing, "%s::for_each_buffer does not class these: %s" % (struct, missing)
    unknown = sorted(set(listed) - set(declared))
    assert not unknown, "%s::for_each_buffer names these, which %s does not declare: %s" % (struct, struct, unknown)
    return body, declared


def test_every_lane_buffer_is_listed_once():
    _, declared = _check("VerifyLane")
    assert len(declared) >= 19


def test_every_context_buffer_is_listed_once_with_its_class():
    body, declared = _check("dsm_ctx")
    assert len(declared) >= 74
    cls = dict(_listed_bufs(body))
    # the chunk outputs the planners size under the budget are scratch; images, the guided matcher's and EstimateMultiple's
    # per-pair state and every result are resident
    for n in ("d_m", "d_ms", "d_entries", "d_vscratch"):
        assert cls[n] is True, n
    for n in ("d_desc", "d_stage", "d_matches", "d_inl_compact", "d_g_m", "d_g_inl", "d_mm_matches[1]", "d_mm_total"):
        assert cls[n] is False, n
    fn = body[body.index("void for_each_buffer("):]
    assert re.search(r"for \(VerifyLane& L : lanes\) L\.for_each_buffer\(\[&f\]\(DevBuf& b\) \{ f\(b, true\); \}\);", fn), \
        "the lanes' buffers are scratch"
