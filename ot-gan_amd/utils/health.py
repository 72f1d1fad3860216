"""--health_every: what a training step looks like numerically, every N steps (nothing the reference computes).

A reported step writes one record: the norm of the summed gradient, of the parameters and of the update of the network it
trains, per variable and in total (ops.tensor_health: one fused pass over the gradients, one over the parameters and their
copy from before the optimiser); how much of every gradient lies where the split-precision engine loses it (`below`); and
how far the Sinkhorn plans of the step are from their column marginals (ops.plan_marginals on the plans of the step's
log-kernels, solved once more through the staged entry points).  trainer.OTGAN.step produces the records, train.main
appends them to <save_dir>/health.jsonl and prints `summary_line` once per epoch.

Definitions (restated in numpy in tests/health_ref.py):
    due(step, every, period)   which steps report: the multiples of `every`, each followed by the first later step of the
                               other kind, so that every report holds a critic and a generator step
    below(hist, bits)          the share of the finite non-zero elements whose fp32 exponent lies `bits` or more below the
                               largest occupied one.  The convolution and matching GEMMs split an operand into two scaled
                               fp16 pieces under a per-tensor amax scale: 11 bits per piece, 22 in all (PIECE_BITS,
                               OPERAND_BITS).  An element 11 or more below the largest lives in the second piece alone; one
                               22 or more below is not represented.
"""
import json
import math

PIECE_BITS, OPERAND_BITS = 11, 22
TWO_BATCH_PROBLEMS = ("a1a2", "b2b1", "a1b1", "a1b2", "a2b1", "a2b2")      # the reference's order, utils/matching.py:41-43
SINGLE_BATCH_PROBLEMS = ("aa", "bb", "ab")                                 # utils/matching.py:99-104


def check_every(every):
    """--health_every as an int >= 0; anything else is a ValueError."""
    if isinstance(every, bool) or int(every) != every or every < 0:
        raise ValueError("--health_every %r: a step count, 0 = off" % (every,))
    return int(every)


def kind_of(step, period):
    return "disc" if step % period == 0 else "gen"


def due(step, every, period):
    """Is step `step` (the trainer's step counter before the step; kinds: critic at step % period == 0, generator otherwise)
    reported?  The multiples of `every` are, and so is the first step after such a multiple that has the other kind.  Pure."""
    if every <= 0:
        return False
    if step % every == 0:
        return True
    if period < 2:
        return False                  # one kind of step only
    anchor = step - step % every
    kind = kind_of(anchor, period)
    if kind_of(step, period) == kind:
        return False
    return all(kind_of(s, period) == kind for s in range(anchor + 1, step))


def below(hist, bits):
    """hist: 256 counts by biased fp32 exponent (bucket 0: denormals) -> the share of them `bits` or more buckets below the
    largest occupied bucket; 0.0 for an empty histogram."""
    count, total = below_counts(hist, bits)
    return count / total if total else 0.0


def below_counts(hist, bits):
    h = [int(c) for c in hist]
    total = sum(h)
    if total == 0:
        return 0, 0
    top = max(b for b, c in enumerate(h) if c)
    return sum(h[:max(top - int(bits) + 1, 0)]), total


def _norm(squares):
    return math.sqrt(math.fsum(float(s) for s in squares))


def collect(step, kind, names, grad_out, grad_hist, par_out=None, distance=None, entropy=None, sinkhorn=None, epoch=None):
    """The record of one reported step from the kernels' outputs on the host: grad_out [nvar, 6] / grad_hist [nvar, 256] of
    the summed gradients, par_out [nvar, 6] of the updated parameters against their copy from before the optimiser (None
    when the optimiser did not run: non-finite gradients), in the order of `names`.  `sinkhorn`: the block made by
    `sinkhorn_block`, or None (--no_sinkhorn)."""
    names = list(names)
    assert len(grad_out) == len(grad_hist) == len(names) and (par_out is None or len(par_out) == len(names))
    vars_, b11, b22, nz = {}, 0, 0, 0
    for i, name in enumerate(names):
        g, h = grad_out[i], grad_hist[i]
        c11, tot = below_counts(h, PIECE_BITS)
        c22, _ = below_counts(h, OPERAND_BITS)
        b11, b22, nz = b11 + c11, b22 + c22, nz + tot
        v = {"n": tot + int(g[4]) + int(g[5]), "grad_norm": math.sqrt(float(g[0])), "grad_amax": float(g[1]),
             "grad_zero": int(g[4]), "grad_nonfinite": int(g[5]), "grad_below_11": c11 / tot if tot else 0.0, "grad_below_22": c22 / tot if tot else 0.0,
             "param_norm": None, "param_amax": None, "update_norm": None, "update_amax": None}
        if par_out is not None:
            p = par_out[i]
            v.update(param_norm=math.sqrt(float(p[0])), param_amax=float(p[1]), update_norm=math.sqrt(float(p[2])),
                     update_amax=float(p[3]))
        vars_[name] = v
    rec = {"step": int(step), "epoch": epoch, "kind": kind, "net": "discriminator" if kind == "disc" else "generator",
           "distance": None if distance is None else float(distance), "entropy": None if entropy is None else float(entropy),
           "grad_norm": _norm(g[0] for g in grad_out), "param_norm": None, "update_norm": None, "update_ratio": None,
           "grad_nonfinite": int(sum(int(g[5]) for g in grad_out)),
           "grad_below_11": b11 / nz if nz else 0.0, "grad_below_22": b22 / nz if nz else 0.0,
           "vars": vars_, "sinkhorn": sinkhorn}
    if par_out is not None:
        rec["param_norm"] = _norm(p[0] for p in par_out)
        rec["update_norm"] = _norm(p[2] for p in par_out)
        rec["update_ratio"] = rec["update_norm"] / rec["param_norm"] if rec["param_norm"] > 0 else None
    return rec


def sinkhorn_block(marginals, iters, lam, problems):
    """marginals: [P, 4] from ops.plan_marginals on the host, problems in the reference's order."""
    assert len(marginals) == len(problems)
    return {"iters": int(iters), "lambda": float(lam), "problems": list(problems),
            "row_err_max": [float(r[0]) for r in marginals], "col_err_max": [float(r[2]) for r in marginals],
            "col_err_mean": [float(r[3]) for r in marginals]}


def nonfinite_variables(record):
    """names of the variables whose gradient holds non-finite elements"""
    return [name for name, v in record["vars"].items() if v["grad_nonfinite"]]


def _plain(x):
    """JSON has no NaN or infinity: they are written as null"""
    if isinstance(x, float):
        return x if math.isfinite(x) else None
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


def dumps(record):
    return json.dumps(_plain(record), allow_nan=False, separators=(",", ":"))


def append(path, record):
    """one JSON object per line"""
    with open(path, "a") as f:
        f.write(dumps(record) + "\n")


def read(path):
    with open(path) as f:
        return [json.loads(line) for line in f if line.strip()]


def _fmt(x, spec="%.3e"):
    return "n/a" if x is None else spec % x


def summary_line(last):
    """last: {"gen": record or None, "disc": record or None}, the last reported pair of steps."""
    g, d = last.get("gen") or {}, last.get("disc") or {}
    recs = [r for r in (g, d) if r.get("sinkhorn")]
    sk = max(recs, key=lambda r: r["step"])["sinkhorn"] if recs else None
    col = ("Sinkhorn column error max %s mean %s (L = %d)"
           % (_fmt(max(sk["col_err_max"])), _fmt(math.fsum(sk["col_err_mean"]) / len(sk["col_err_mean"])), sk["iters"])
           if sk else "Sinkhorn column error n/a")
    return ("health: |g| gen %s disc %s, update/param gen %s disc %s, below 22 bits gen %s disc %s, %s"
            % (_fmt(g.get("grad_norm")), _fmt(d.get("grad_norm")), _fmt(g.get("update_ratio")), _fmt(d.get("update_ratio")),
               _fmt(g.get("grad_below_22"), "%.4f"), _fmt(d.get("grad_below_22"), "%.4f"), col))
