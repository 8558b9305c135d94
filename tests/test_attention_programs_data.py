"""CPU: the programs and the models of tests/attention_programs.py -- what tests/test_gpu_attention_programs.py and
tests/gpu_dist_attention_programs_worker.py rely on.  Nothing here runs a kernel: these are conditions on the inputs, held with the
references alone."""
import numpy as np
import pytest

import attention_programs as AP
import call_programs as CP


def _walk_handle():
    """(program, data, model after the last step, [(step, what the model held before it)])"""
    out = []
    for prog in AP.handle_programs():
        pat, data, model = AP.handle_setup(prog)
        seen = []
        for step in prog.steps:
            h = AP.handle_of(step) if step[0] not in AP.CTRL else None
            seen.append((step, dict(cur=model.cur, prev=model.prev, kind=model.values.kind, map=dict(model.map), before=dict(model.map_before),
                                    bounded=AP.bounded(step, model, prog.two_source), handle=h)))
            model.apply(step)
        out.append((prog, data, model, seen))
    return out


def _walk_engine(several):
    out = []
    for prog, n in AP.engine_programs(several):
        pat, data, model = AP.engine_setup(prog, n)
        kinds = []
        for step in prog.steps:
            kinds.append(model.kind())
            model.apply(step)
        out.append((prog, n, model, kinds))
    return out


def test_programs_are_reproducible_literals():
    """a program is a pure function of its seed, and its steps print as literals that evaluate back to themselves"""
    first = [p.steps for p in AP.handle_programs()]
    AP.handle_programs.cache_clear()
    again = AP.handle_programs()
    assert [p.steps for p in again] == first
    for prog in again:
        assert eval(repr(prog.steps)) == prog.steps and len(prog.steps) == AP.HANDLE_STEPS
        env = {}
        exec(AP.literal(prog, 5), env)
        assert tuple(env["steps"]) == prog.steps[:6]
    for several in (False, True):
        first = [p.steps for p, _ in AP.engine_programs(several)]
        AP.engine_programs.cache_clear()
        assert [p.steps for p, _ in AP.engine_programs(several)] == first
        for prog, n in AP.engine_programs(several):
            assert eval(repr(prog.steps)) == prog.steps and len(prog.steps) == AP.ENGINE_STEPS
    assert [p.steps for p, _ in AP.engine_programs(False)] != [p.steps for p, _ in AP.engine_programs(True)]


def test_setups_and_parameters():
    assert len(AP.HANDLE_SETUPS) == AP.HANDLE_PROGRAMS and {s[0] for s in AP.HANDLE_SETUPS} == set(CP.MATRICES)
    assert sum(s[1] for s in AP.HANDLE_SETUPS) * 2 == AP.HANDLE_PROGRAMS, "half of the programs are two-source"
    assert AP.DROPS == (0.0, 0.5, 0.6) and len(set(AP.SEEDS)) == 2 and AP.SEEDS[0] >> 32 and 7 in AP.SEEDS
    for prog, data, model, seen in _walk_handle():
        assert data.rowmapsT[1][1] > data.pat.k and sorted(set(data.rowmapsT[1][0])) == sorted(data.rowmapsT[1][0])
        for step, _ in seen:
            k = step[0]
            assert step[1] in (0, 1, 2)
            if k in AP.ATTN:
                assert step[2] in ("f64", "f32") and step[4] in AP.HEADS and 0 <= step[5] < len(CP.ATTN_WIDTHS)
            if k in AP.GATS:
                assert step[2] in ("f64", "f32") and step[4] in AP.HEADS and step[5] in AP.GAT_DV and step[6] in AP.DROPS and step[7] in AP.SEEDS
                assert step[5] <= 512, "one head stays under the backward caps"
            if k == "mask":
                assert step[3] in AP.HEADS and step[4] in AP.DROPS[1:] and step[5] in AP.SEEDS
    assert AP.ENGINE_PROGRAMS == len(AP.ENGINE_SETUPS) == len(AP.ENGINE_LAYOUTS) and [n for _, n in AP.ENGINE_SETUPS] == [24, 40, 64, 26]
    assert set(AP.ENGINE_LAYOUTS) == {"balanced", "a rank without rows of A", "a rank without rows of B"}
    assert AP.heads_of(26) == (1, 2) and AP.heads_of(24) == AP.heads_of(40) == AP.heads_of(64) == (1, 2, 4)


def test_the_mask_model_is_dropout_ref_s_key():
    """attention_programs.mask_of on A is dropout_ref.mask_csr on the codes as stored; on A^T it flags the same edges as A on a
    one-source pair without row maps (csrc/dropout.h: both handles draw the same bit), and differs under either handle's row map"""
    pat = AP.pattern("rect", False)
    data = AP.Data(pat, 5)
    a = AP.mask_of(data, "A", 0, 2, 0.5, 7)
    t = AP.mask_of(data, "T", 0, 2, 0.5, 7)
    assert np.array_equal(a[pat.tmap], t) and 0.4 < a.mean() < 0.6
    assert AP.mask_change(data, "A", 1, 0, 2, 0.5, 7) > 0.25 and AP.mask_change(data, "T", 2, 1, 2, 0.5, 7) > 0.25
    two = AP.Data(AP.pattern("rect", True), 5)
    codes = two.pat.codes
    assert (codes < 0).any() and np.array_equal(AP.mask_of(two, "A", 0, 1, 0.6, 7)[:, 0],
                                                AP.DR.keep(7, two.pat.rows, codes.astype(np.int64) & 0xFFFFFFFF, 0, 0.6))


# ---- the handle programs -----------------------------------------------------------------------------------------------------------

def test_handle_coverage():
    walks = _walk_handle()
    kinds, pairs, log = set(), set(), []
    by = {}
    for prog, data, model, seen in walks:
        ks = [AP.kind_of(s) for s, _ in seen]
        kinds |= set(ks)
        pairs |= set(zip(ks, ks[1:]))
        log += model.log
        for step, _ in seen:
            k = AP.kind_of(step)
            if step[0] in AP.ATTN + AP.GATS:
                by.setdefault(("dtype", k), set()).add(step[2])
                by.setdefault(("H", k), set()).add(step[4])
            d = AP.dropout_of(step)
            if d is not None:
                by.setdefault(("rate", k), set()).add(d[1])
                by.setdefault(("seed", k), set()).add(d[2])
    assert kinds == set(AP.HANDLE_KINDS), ("kinds that never occur", set(AP.HANDLE_KINDS) - kinds)
    missing = sorted(AP.required_pairs() - pairs)
    assert not missing, ("ordered pairs of a control and a dropout kind that are never adjacent", missing)
    built = {ev[1:] for ev in log if ev[0] == "built"}
    missing = [(h, s, b) for h in "AT" for s in CP.SITUATIONS for b in ("fused", "spmm32") if (h, s, b) not in built]
    assert not missing, ("val32 never built on this handle, in this situation, by this builder", missing)
    read = {(ev[1], ev[2], AP.family_of(ev[3])) for ev in log if ev[0] == "read_after"}
    missing = [(h, u, f) for h in "AT" for u in ("host", "dev") for f in ("gat", "gatv2") if (h, u, f) not in read]
    assert not missing, ("val32 never read after this kind of update by this family's bias step", missing)
    states = {ev[1:] for ev in log if ev[0] == "drop"}
    missing = [(k, s) for k in AP.DROP_KINDS for s in ("set", "changed", "cleared")
               if (k, "T" if (k == "maskT" or k.split("/")[0] in AP.ON_T) else "A", s) not in states]
    assert not missing, ("dropout kinds that never run in this state of their handle's row map", missing)
    for k in AP.DROP_KINDS:
        assert by["rate", k] == set(AP.DROPS[1:]) and by["seed", k] == set(AP.SEEDS), (k, by["rate", k], by["seed", k])
    for k in AP.ATTN + AP.GATS + tuple(x for x in AP.DROP_KINDS if "/" in x):
        assert by["dtype", k] == {"f64", "f32"}, (k, by["dtype", k])
        assert by["H", k] == set(AP.HEADS), (k, by["H", k])


def test_handle_sensitivity_of_the_masks():
    """for every dropout step: the numpy mask under its handle's current row map differs from the mask under the map before it (no
    map where there was none) in at least a quarter of its entries"""
    total = held = 0
    for prog, data, model, seen in _walk_handle():
        for step, was in seen:
            d = AP.dropout_of(step)
            if d is None:
                continue
            total += 1
            h = was["handle"]
            if was["before"][h] is None:
                continue                # the handle's row map has never changed: there is no other mask to take this one for
            share = AP.mask_change(data, h, was["map"][h], was["before"][h], *d)
            assert share >= 0.25, (prog.seed, step, share)
            held += 1
    print("dropout steps: %d, of them %d after a change of their handle's row map" % (total, held))
    assert held * 4 >= total * 3


def test_handle_sensitivity_of_the_bias():
    """for every bias step checked by bounds: the forward's reference under the current value set differs from the reference under
    the previous set by more than the bound in at least half of the rows"""
    count = 0
    for prog, data, model, seen in _walk_handle():
        done = {}
        for step, was in seen:
            if step[0] not in AP.ATTN + AP.GATS or not step[3] or not was["bounded"]:
                continue
            assert was["kind"] == "R" and was["prev"] is not None
            fwd = {"bwd_q": "attn", "bwd_kv": "attn"}.get(step[0], step[0].split("_")[0])
            key = (fwd, step[2], step[4], step[5], was["cur"], was["prev"])
            if key not in done:
                done[key] = AP.bias_change(data, (fwd,) + tuple(step[1:]), was["cur"], was["prev"])
            assert done[key] >= 0.5, (prog.seed, step, done[key])
            count += 1
    print("bias steps checked by bounds: %d" % count)
    assert count >= 8


def test_handle_counts():
    steps = bitwise = bounded = 0
    for prog, data, model, seen in _walk_handle():
        for step, was in seen:
            steps += 1
            bitwise += step[0] not in AP.CTRL
            bounded += was["bounded"] or (step[0] == "spmm32" and was["kind"] != "E32")
    print("attention handle programs: %d steps, %d compared bit for bit with a fresh pair, %d held to bounds" % (steps, bitwise, bounded))
    assert bounded * 3 >= bitwise, "a third of the call steps are held to bounds"


# ---- the engine programs -----------------------------------------------------------------------------------------------------------

def _host_p(step, H=None, dtype=None):
    """a fused forward with a host p_out (of H heads, of this dtype)"""
    return step[0] in ("attn", "gat", "gatv2") and step[5] == "host" and (H is None or step[4] == H) and (dtype is None or step[2] == dtype)


def _host_sddmm(step):
    return step[0] == "sddmm" and step[4] == "host"


def _ordered(steps, *preds):
    """whether steps satisfying the predicates occur in this order"""
    j = 0
    for s in steps:
        if j < len(preds) and preds[j](s):
            j += 1
    return j == len(preds)


@pytest.mark.parametrize("several", (False, True))
def test_engine_conditions(several):
    walks = _walk_engine(several)
    other = {"f64": "f32", "f32": "f64"}
    shapes = {dt: set() for dt in other}
    between = {dt: set() for dt in other}
    staging, backward, first, built, bias_after = set(), set(), set(), set(), set()
    kinds = set()
    for prog, n, model, vkinds in walks:
        steps = prog.steps
        kinds |= {s[0] for s in steps}
        for s, vk in zip(steps, vkinds):
            assert s[0] in AP.ENGINE_KINDS
            if s[0] in ("attn", "attn_bwd", "gat", "gatv2"):
                assert n % s[4] == 0 and s[4] in AP.HEADS
            if several and s[0] == "attn_bwd" and s[3]:
                assert vk == "R", "at several ranks the backward takes the values under the R set only"
        for dt in other:
            last, earlier = None, set()
            for i, s in enumerate(steps):
                if s[0] != "gat" or s[2] != dt:
                    continue
                if last is not None and s[4] != steps[last][4]:
                    H0 = steps[last][4]
                    shapes[dt].add("increase" if s[4] > H0 else "decrease")
                    if s[4] in earlier:
                        shapes[dt].add("return")
                    for b in steps[last + 1:i]:
                        between[dt].add("gat of the other dtype" if (b[0] == "gat" and b[2] == other[dt]) else
                                        "sddmm with a host out" if _host_sddmm(b) else b[0])
                earlier.add(s[4])
                last = i
            if _ordered(steps, lambda s: _host_p(s, 4), _host_sddmm, lambda s: _host_p(s, 4)):
                staging.add("sddmm")
            if _ordered(steps, lambda s: _host_p(s, 4, dt), lambda s: _host_p(s, 1, other[dt]), lambda s: _host_p(s, 4, dt)):
                staging.add("one head of the other dtype")
            bw = lambda H: (lambda s: s[0] == "attn_bwd" and s[2] == dt and s[4] == H)
            if _ordered(steps, bw(4), bw(1), bw(4)):
                backward.add(dt)
        first.add(model.first_uploader)
        built |= {ev[1:] for ev in model.log if ev[0] == "built" and ev[1] in ("gat", "gatv2")}
        bias_after |= {ev[1:] for ev in model.log if ev[0] == "bias_after"}
    assert kinds == set(AP.ENGINE_KINDS), set(AP.ENGINE_KINDS) - kinds
    for dt in other:
        assert shapes[dt] == {"increase", "decrease", "return"}, (dt, shapes[dt])
        assert between[dt] >= {"gat of the other dtype", "exec", "attn", "sddmm with a host out", "update_dev"}, (dt, between[dt])
    assert staging == {"sddmm", "one head of the other dtype"}, staging
    assert backward == {"f64", "f32"}, backward
    assert first >= set(AP.FIRST_UPLOADER), first
    assert built == {(p, s) for p in ("gat", "gatv2") for s in CP.SITUATIONS}, built
    assert bias_after == {(p, u) for p in ("gat", "gatv2") for u in ("host", "dev")}, bias_after


def test_engine_counts():
    for several in (False, True):
        steps = bitwise = bounded = 0
        for prog, n, model, vkinds in _walk_engine(several):
            for s, vk in zip(prog.steps, vkinds):
                steps += 1
                if s[0] in ("attn", "gat", "gatv2", "softmax", "softmax_bwd", "attn_bwd"):
                    bitwise += 1
                    bounded += several and s[0] == "attn_bwd"
                elif s[0] in ("exec", "exec_t", "sddmm"):
                    exact = (s[0] == "sddmm" and s[3] == 0) or CP.exact_in(vk, s[2])
                    bitwise += exact
                    bounded += not exact
        print("attention engine programs at %s: %d steps, %d compared bit for bit, %d held to bounds"
              % ("several ranks" if several else "one rank", steps, bitwise, bounded))
        assert bitwise * 2 >= steps


def test_partitions():
    """the layouts of the several-rank family: a partition of the rows, with the hole where the layout says"""
    for world in (2, 4):
        for layout in set(AP.ENGINE_LAYOUTS):
            for name in CP.MATRICES:
                pat = AP.pattern(name, False)
                rb, bd = AP.partition(layout, pat.rp, world, pat.k)
                assert rb[0] == 0 and rb[-1] == pat.m and (np.diff(rb) >= 0).all() and len(rb) == world + 1
                assert bd[0] == 0 and bd[-1] == pat.k and (np.diff(bd) >= 0).all() and len(bd) == world + 1
                assert (np.diff(rb) == 0).any() == (layout == "a rank without rows of A")
                assert (np.diff(bd) == 0).any() == (layout == "a rank without rows of B")
