"""The refusals of the guidance keywords, whole message by whole message.  The validation tests of the keywords match fragments
(`name + ".*torch_cpu"`); the messages are assembled from one template per precondition and a table of sentence tails
(guidance.PRECONDITION_TAILS), so what can go wrong is the exact wording, the order in which two bad keywords are looked at, and which
entry point still takes which name.  Every case below goes through a public entry point, on a model that was never moved to a GPU
(nothing can run), and its "ExcType: message" equals the string stored in tests/golden/guidance_messages.json.

The stored strings were recorded from the commit BEFORE the checks moved to guidance.py, never from the code under test:

    python -m tests.test_guidance_messages --record tests/golden/guidance_messages.json        # in a checkout of that commit

which refuses to write a file in which a case raised nothing or anything but a ValueError or TypeError: such a case is a mistake in
the table below, not something to skip."""
import json
import os

import torch

from ccdm_stochastic_segmentation_amd.distributed import sample_sharded
from tests.sampler_util import FREE, H, ROOT, T_STRIDED, W, small_model

GOLDEN = os.path.join(ROOT, "tests", "golden", "guidance_messages.json")
N, K = 2, 3
KEYWORDS = ("known_labels", "resample", "evidence", "temperature", "truncation", "views", "tiles")


# ------------------------------------------------------------------------------------------------ inputs and entry points
def inputs():
    x = torch.nn.functional.one_hot(torch.zeros((N, H, W), dtype=torch.int64), K).permute(0, 3, 1, 2).float()
    known = torch.full((N, H, W), FREE, dtype=torch.int64)
    known[:, :4] = 1
    return dict(x=x, cond=torch.zeros(N, 1, H, W), known=known, evidence=torch.full((N, K, H, W), 0.5), t_each=torch.full((N,), 3.0),
                features=torch.zeros(N, 4, 8, 8))


IN = inputs()
# a good value of every keyword (`tiles`: one tile that is the canvas)
GOOD = dict(known_labels=IN["known"], resample=(2, 2), evidence=IN["evidence"], temperature=0.7, truncation=0.9, views=("hflip",),
            tiles=(32, 32, 32, 32))


def models():
    """variant -> model: "plain"; "logits" (softmax_output: no); "features" (takes a feature_condition: only the checks read it)"""
    out = {"plain": small_model(K)[0].eval(), "logits": small_model(K, softmax_output=False)[0].eval(), "features": small_model(K)[0].eval()}
    out["features"].unet.spec.feature_condition_idx = [1]
    return out


def multi(entry, **more):
    return lambda m, kw: getattr(m, entry)(IN["cond"], num_evaluations=2, t=T_STRIDED, **more, **kw)


def submit(guided):
    def call(m, kw):
        q = m.sampling_queue(4, (1, H, W), guided=guided)
        try:
            return q.submit(IN["cond"], **kw)
        finally:
            assert q._engine is None, "a queue engine was built"
    return call


# entry -> (call(model, keywords), train mode)
ENTRIES = {
    "call": (lambda m, kw: m(IN["x"], IN["cond"], t=T_STRIDED, **kw), False),
    "call_with_features": (lambda m, kw: m(IN["x"], IN["cond"], IN["features"], t=T_STRIDED, **kw), False),
    "call_validation": (lambda m, kw: m(IN["x"], IN["cond"], t=IN["t_each"], validation=True, **kw), False),
    "call_train": (lambda m, kw: m(IN["x"], IN["cond"], t=IN["t_each"], **kw), True),
    "forward_denoising": (lambda m, kw: m.forward_denoising(IN["x"], IN["cond"], None, 10004, **kw), False),
    "forward_denoising_train": (lambda m, kw: m.forward_denoising(IN["x"], IN["cond"], None, 10004, **kw), True),
    "predict_multiple": (multi("predict_multiple", voting="majority"), False),
    "predict_multiple_batched": (multi("predict_multiple", voting="confidence", batched=True), False),
    "predict_modes": (multi("predict_modes", modes=1), False),
    "predict_findings": (multi("predict_findings"), False),
    "sample_sharded": (lambda m, kw: sample_sharded(m, IN["x"], IN["cond"], None, T_STRIDED, **kw), False),
    "submit": (submit(False), False),
    "submit_guided": (submit(True), False),
    "label_bound": (lambda m, kw: m.label_bound(IN["known"], IN["cond"], **kw), False),
}
SAMPLING = ("call", "forward_denoising", "predict_multiple", "predict_multiple_batched", "predict_modes", "predict_findings", "sample_sharded")


# ------------------------------------------------------------------------------------------------ the table
def cases():
    """id -> (entry, model variant, rng, keywords)"""
    out = {}

    def add(group, entry, keywords, variant="plain", rng="philox", tag=None):
        key = f"{group}/{entry}/{tag or '+'.join(keywords)}"
        assert key not in out, key
        out[key] = (entry, variant, rng, keywords)

    def good(*names):
        return {n: GOOD[n] for n in names}

    # each keyword alone against each precondition it has (`resample` meets rng = "torch_cpu" only with the known labels it needs)
    for name in KEYWORDS:
        for entry in ("call_train", "call_validation") + (("forward_denoising_train",) if name not in ("known_labels", "resample") else ()):
            add("not_sampling", entry, good(name))
        for entry in SAMPLING:
            add("torch_cpu", entry, good(name, "known_labels") if name == "resample" else good(name), rng="torch_cpu", tag=name)
            if name not in ("known_labels", "resample"):
                add("logits", entry, good(name), variant="logits")
    add("torch_cpu", "label_bound", {}, rng="torch_cpu", tag="label_bound")
    add("logits", "label_bound", {}, variant="logits", tag="label_bound")
    # the pairwise refusals
    for entry in ("call", "predict_multiple", "predict_modes", "sample_sharded"):
        for pair in (("tiles", "views"), ("tiles", "known_labels"), ("tiles", "resample"), ("views", "known_labels"), ("views", "resample"),
                     ("resample",)):
            add("pairs", entry, good(*pair))
    # one bad value per value check
    ev, known = IN["evidence"], IN["known"]
    nan, outside, ruled_out, bad_class = ev.clone(), ev.clone(), ev.clone(), known.clone()
    nan[0, 0, 0, 0], outside[1, 2, 3, 4], bad_class[1, 5, 5] = float("nan"), 1.5, 7
    ruled_out[0, :, 2, 2] = 0.0
    bad_values = {
        "tiles": [("three", (32, 32, 16)), ("float", (32, 32, 16.0, 8)), ("bool", (32, 32, True, 8)), ("stride", (32, 32, 0, 8)),
                  ("beyond", (32, 32, 16, 40)), ("canvas", (64, 32, 16, 8))],
        "views": [("string", "hflip"), ("unknown", ("flip", 3)), ("duplicate", ("hflip", "vflip", "hflip"))],
        "temperature": [("low", 0.01), ("bool", True), ("nan", float("nan"))],
        "truncation": [("zero", 0.0), ("high", 1.5), ("string", "0.5")],
        "evidence": [("integer", ev.long()), ("shape", ev[:, :, :, 1:]), ("nan", nan), ("outside", outside), ("ruled_out", ruled_out),
                     ("array", ev.numpy())],
        "resample": [("one", (2,)), ("negative", (-1, 2)), ("zero", (2, 0)), ("bool", (True, 2)), ("float", (2.0, 2))],
        "known_labels": [("float", known.float()), ("shape", known[:, 1:]), ("class", bad_class), ("bool", known > 0)],
    }
    for name, values in bad_values.items():
        for entry in ("call", "predict_multiple", "predict_findings") + (("submit_guided",) if name in ("evidence", "known_labels", "temperature",
                                                                                                        "truncation") else ()):
            for tag, value in values:
                add("value", entry, dict(good("known_labels") if name == "resample" else {}, **{name: value}), tag=f"{name}_{tag}")
    for name in ("tiles", "views"):          # a model that takes features needs one leading entry per tile or view
        add("value", "call_with_features", good(name), variant="features", tag=f"{name}_features")
    # two bad keywords: the sampling order tiles, views, temperature / truncation, evidence, resample, known_labels names the first ...
    first_bad = dict(tiles=(32, 32, 16), views=("flip",), temperature=0.01, truncation=1.5, evidence=outside, resample=(2,), known_labels=bad_class)
    for a, b in (("tiles", "views"), ("views", "temperature"), ("temperature", "truncation"), ("truncation", "evidence"),
                 ("evidence", "resample"), ("resample", "known_labels")):
        for entry in ("call", "predict_multiple_batched", "predict_modes"):
            add("two_bad", entry, {a: first_bad[a], b: first_bad[b]})
    # ... and the order of a training or validation call is evidence, tiles, temperature / truncation, views, known_labels, resample
    for a, b in (("evidence", "tiles"), ("tiles", "temperature"), ("tiles", "truncation"), ("temperature", "views"), ("truncation", "views"),
                 ("views", "known_labels"), ("known_labels", "resample")):
        for entry in ("call_train", "call_validation"):
            add("two_not_sampling", entry, good(a, b))
    add("two_not_sampling", "call_train", dict(good("evidence"), tiles=(32, 32, 16)), tag="evidence+bad_tiles")      # evidence refuses the call first
    add("two_not_sampling", "call_train", dict(good("views"), tiles=(32, 32, 16)), tag="views+bad_tiles")            # tiles looks at its integers first
    # names no entry point takes, and what a queue does not take
    for entry in ("predict_modes", "predict_findings", "sample_sharded", "submit", "submit_guided"):
        add("unknown", entry, dict(guide=1))
        add("unknown", entry, dict(good("temperature"), known_label=IN["known"]), tag="temperature+known_label")
    for name in KEYWORDS:
        add("queue", "submit", good(name))
    for name in ("views", "tiles", "resample"):
        add("queue", "submit_guided", good(name))
    add("queue", "submit_guided", dict(good("temperature"), views=("hflip",), guide=1), tag="temperature+views+guide")
    return out


def outcomes():
    """id -> "ExcType: message" (or "no exception") of every case, and that nothing ran in any of them."""
    ms = models()
    got = {}
    for key, (entry, variant, rng, keywords) in cases().items():
        call, train = ENTRIES[entry]
        m = ms[variant]
        m.rng = rng
        m.train(train)
        try:
            call(m, keywords)
            got[key] = "no exception"
        except Exception as e:       # noqa: BLE001   (the type is part of what is compared)
            got[key] = f"{type(e).__name__}: {e}"
        finally:
            m.rng = "philox"
            m.eval()
        assert m.philox_call == 0 and m.bound_call == 0 and m._engines == {}, f"{key}: something ran"
    return got


# ------------------------------------------------------------------------------------------------ the tests
def test_the_stored_messages_are_refusals_of_every_case():
    """The file holds one string per case of the table, and each is a ValueError or a TypeError."""
    want = json.load(open(GOLDEN))
    assert sorted(want) == sorted(cases())
    assert all(v.startswith(("ValueError: ", "TypeError: ")) for v in want.values())


def test_every_refusal_keeps_its_type_and_message():
    want = json.load(open(GOLDEN))
    got = outcomes()
    wrong = {k: (got[k], want.get(k)) for k in got if got[k] != want.get(k)}
    assert not wrong, "\n".join(f"{k}\n   now: {g}\n  then: {w}" for k, (g, w) in wrong.items())


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", required=True, metavar="PATH")
    path = ap.parse_args().record
    seen = outcomes()
    no_refusal = {k: v for k, v in seen.items() if not v.startswith(("ValueError: ", "TypeError: "))}
    if no_refusal:
        raise SystemExit("not written, these cases are no refusals:\n" + "\n".join(f"{k}: {v}" for k, v in no_refusal.items()))
    with open(path, "w") as f:
        json.dump(seen, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(seen)} cases -> {path}")
