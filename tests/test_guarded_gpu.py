"""-m gpu: no result depends on what memory held before (tests/guard.py).

Every case runs eagerly twice in this process - once with every `torch.empty` buffer filled with the poison word
0x7FC0BEEF (pattern A), once with zeros (pattern B), both between red zones - and every tensor an entry point of the
binding took or returned must hold the same BITS after both runs.  The library uses no floating-point atomics (DESIGN.md:
"deterministic slab reduction, no atomics") and the suite already asserts bit equality between eager and replayed runs,
so equality is exact: an output element that is never written, or a value computed from memory the kernel does not own,
differs between the two runs.  The kernel-level cases are the launches of tests/test_kernels_gpu.py (and of the other
"against definition" tests) at their edge shapes - ragged M, Cin not a multiple of the tile, V = 1, N = 1 - so each also
passes its own comparison with the definition under both patterns.

Input-side variant (conv, aggconv, wgrad, wgrad_many): the operands are handed over as guarded tensors too (storage offset 0, pattern A
directly in front of and behind them) and the results must equal the run on plain operands bit for bit: any over-read - in
front of a row (KgConvGroup.x_lead), past the end of `add` / `mask` / `x` - that reaches the output is a NaN there."""
import collections
import inspect

import pytest
import torch

import kinetic_gan_amd  # noqa: F401
from kinetic_gan_amd import _native as nv
from kinetic_gan_amd import disc_trunk, gen_trunk, metrics
from kinetic_gan_amd._native import TAP_CHANBLOCK, TAP_TIME
from kinetic_gan_amd.sample import Sampler
from kinetic_gan_amd.wgan_gp import Trainer
from oracle import prim_ref
from oracle.fill import rand_inputs, rand_noise
from tests import guard
from tests import test_agg_forms_gpu as ta
from tests import test_conv_forms_gpu as tf
from tests import test_d0_fused_gpu as td
from tests import test_ema_gpu as te
from tests import test_kernels_gpu as tk
from tests import test_sampler_gpu as ts
from tests import test_train_gpu as tt
from tests import test_wgrad_tiles_gpu as tw
from tests.guard import PATTERN_A, Guard
from tests.util import CFG, ReloadingEnv, build_pair

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

ENTRY = [n for n in prim_ref.NAMES + ["aggconv_label", "adam_step_ema", "step_inputs", "sample_inputs", "trunc_lerp",
                                      "loss_append", "bn_eval_coef", "genblock_infer", "mmd", "conv_pack"] if hasattr(nv, n)]
SCRATCH_KEYS = {"ws", "keep", "args"}          # workspaces inside deferred-job records: scratch, not results
GUARDED_OPERANDS = ("conv", "aggconv", "wgrad", "wgrad_many")
# disc_trunk._d0_fused_route takes the fused block-0 route only while these two are the library's own functions (the CPU
# tests swap in emulations): the model-level cases leave them unwrapped, so the production route runs
IDENTITY_CHECKED = ("label_bias_fwd", "aggconv")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    assert torch.cuda.is_available()
    nv.load_library()


Env = ReloadingEnv      # tests/test_kernels_gpu.py's `monkeypatch`: the library reads its KG_* switches when told to


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view(torch.uint8).cpu() if t.numel() else torch.empty(0, dtype=torch.uint8)


def guarded_copy(t):
    """`t` again with pattern A directly around it: same shape and strides, the same data-pointer alignment modulo 16 bytes
    (the launchers pick 16-byte loads by it), storage offset 0 - lead 0 - for every 16-byte-aligned operand"""
    if t is None or not t.is_cuda or t.numel() == 0:
        return t
    like = torch.empty_like(t, device="meta")
    if like.stride() != t.stride():            # not dense (a slice of a larger tensor): left alone
        return t
    lead = (t.data_ptr() % 16) // t.element_size()
    flat = guard.empty(lead + t.numel(), dtype=t.dtype, device=t.device)
    out = flat.as_strided(t.size(), t.stride(), lead) if lead else flat.as_strided(t.size(), t.stride())
    out.copy_(t)
    assert out.data_ptr() % 16 == t.data_ptr() % 16 and (lead or out.storage_offset() == 0)
    return out


def _guard_operands(name, fn, args, kwargs):
    ba = inspect.signature(fn).bind(*args, **kwargs)
    a = ba.arguments
    if name == "conv":
        a["groups"] = [g._replace(x=guarded_copy(g.x), w=guarded_copy(g.w), vmap=guarded_copy(g.vmap)) for g in a["groups"]]
        for k in ("bias0", "bias1", "add", "mask"):
            if a.get(k) is not None:
                a[k] = guarded_copy(a[k])
    elif name == "aggconv":
        for k in ("x", "A", "nbr", "w", "add"):
            if a.get(k) is not None:
                a[k] = guarded_copy(a[k])
    elif name == "wgrad":
        for k in ("g", "x", "vmap"):
            if a.get(k) is not None:
                a[k] = guarded_copy(a[k])
        if a.get("extra"):
            a["extra"] = [(guarded_copy(g), guarded_copy(x)) for g, x in a["extra"]]
    elif name == "wgrad_many":
        a["jobs"] = [dict(j, g=guarded_copy(j["g"]), x=guarded_copy(j["x"]), vmap=guarded_copy(j.get("vmap")),
                          extra=[(guarded_copy(g), guarded_copy(x)) for g, x in j.get("extra", ())]) for j in a["jobs"]]
    return ba.args, ba.kwargs


class Recorder:
    """Wraps the binding's entry points: remembers every device tensor they take or return (in order of first sight)
    and, when the case ends, the bits each of them holds."""

    def __init__(self, guard_operands=False, outputs_only=False, count_only=False):
        self.seen, self.ids, self.calls = [], set(), collections.Counter()
        self.guard_operands, self.outputs_only, self.count_only = guard_operands, outputs_only, count_only
        self.saved = {}

    def _walk(self, o, what):
        if isinstance(o, torch.Tensor):
            if o.is_cuda and id(o) not in self.ids:
                self.ids.add(id(o))
                self.seen.append((what, o))
        elif isinstance(o, dict):
            for k, v in o.items():
                if k not in SCRATCH_KEYS:
                    self._walk(v, "%s[%r]" % (what, k))
        elif isinstance(o, (list, tuple)):
            for i, v in enumerate(o):
                self._walk(v, "%s[%d]" % (what, i))

    def _wrap(self, name, fn):
        def wrapped(*args, **kwargs):
            n = self.calls[name]
            self.calls[name] += 1
            if self.count_only:                # (model level: what the case returns is compared, the launches are counted)
                return fn(*args, **kwargs)
            if not self.outputs_only:          # (with guarded operands the operands are other tensors: results only)
                self._walk(args, "%s#%d args" % (name, n))
                self._walk(kwargs, "%s#%d kwargs" % (name, n))
            if self.guard_operands and name in GUARDED_OPERANDS:
                args, kwargs = _guard_operands(name, fn, args, kwargs)
            res = fn(*args, **kwargs)
            self._walk(res, "%s#%d result" % (name, n))
            if name == "wgrad_many":           # (returns nothing: its results are the jobs' destinations)
                self._walk([j["out"] for j in (args[0] if args else kwargs["jobs"])], "%s#%d out" % (name, n))
            return res
        return wrapped

    def __enter__(self):
        for name in ENTRY:
            if self.count_only and name in IDENTITY_CHECKED:
                continue
            self.saved[name] = getattr(nv, name)
            setattr(nv, name, self._wrap(name, self.saved[name]))
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(nv, name, fn)
        return False

    def snapshot(self, extra=()):
        torch.cuda.synchronize()
        for i, t in enumerate(extra):
            self._walk(t, "returned[%d]" % i)
        return [(what, tuple(t.shape), t.dtype, _bits(t)) for what, t in self.seen]


def run_case(body, pattern, guard_operands=False, outputs_only=False, count_only=False):
    """`body()` under one pattern; returns (snapshots, calls per entry point, the guard)"""
    torch.manual_seed(1234)
    with Guard(pattern) as g:
        with Recorder(guard_operands, outputs_only, count_only) as rec:
            extra = body()
            snap = rec.snapshot(extra if isinstance(extra, (list, tuple)) else () if extra is None else (extra,))
    return snap, rec.calls, g


def same_bits(sa, sb, what_a="pattern A", what_b="pattern B"):
    assert [(s[0], s[1], s[2]) for s in sa] == [(s[0], s[1], s[2]) for s in sb], "the two runs made different calls"
    bad = []
    for (what, shape, dtype, a), (_, _, _, b) in zip(sa, sb):
        if not torch.equal(a, b):
            es = torch.empty(0, dtype=dtype).element_size()
            ne = (a != b).view(-1, es).any(1).nonzero().reshape(-1)
            word = a[:a.numel() // 4 * 4].view(torch.int32) if a.numel() >= 4 else a.new_empty(0, dtype=torch.int32)
            bad.append("%s %s %s: %d of %d elements differ, first at flat index %d, last at %d; %d words of the first run are "
                       "the poison 0x%08X" % (what, shape, dtype, ne.numel(), a.numel() // es, int(ne[0]), int(ne[-1]),
                                              int((word == PATTERN_A).sum()), PATTERN_A))
    assert not bad, "%s and %s differ:\n  " % (what_a, what_b) + "\n  ".join(bad)


def ab(body, expect=(), count_only=False):
    """the case under pattern A and under pattern B: same bits everywhere; `expect`: entry points that must have run"""
    sa, calls, ga = run_case(body, "A", count_only=count_only)
    sb, _, gb = run_case(body, "B", count_only=count_only)
    for name in expect:
        assert calls[name] > 0, "%s was not launched by this case (%s)" % (name, dict(calls))
    assert sa and ga.allocations > 0 and gb.allocations == ga.allocations
    same_bits(sa, sb)
    ga.calls = calls
    return ga


# ---- kernel level ---------------------------------------------------------------------------------------------------------
def _k(fn, *args, expect=(), env=None, **kw):
    return (fn, args, kw, tuple(expect), env or {})


KERNEL_CASES = {
    # kg_conv: every plan tile the KG_CONV_* switches reach (each case asserts the plan through last_conv_plan itself)
    "conv tiles 0-4,9 + K-split, ragged M / Cin / columns": _k(tk.test_conv_forced_tiles_on_plane_tensors, 5, 20, 33, 7, 5, 1, TAP_TIME, False, expect=["conv"]),
    "conv tiles, 3 taps, Cin 17, M 70": _k(tk.test_conv_forced_tiles_on_plane_tensors, 3, 17, 70, 9, 25, 3, TAP_TIME, False, expect=["conv"]),
    "conv tiles, transposed, V = 1": _k(tk.test_conv_forced_tiles_on_plane_tensors, 70, 40, 96, 64, 1, 3, TAP_TIME, True, expect=["conv"]),
    "conv tiles, channel-block taps": _k(tk.test_conv_forced_tiles_on_plane_tensors, 64, 63, 32, 64, 11, 3, TAP_CHANBLOCK, False, expect=["conv"]),
    "conv tile 11 (tiny-channel kernel), out_t0 / out_tstride": _k(tk.test_conv_tiny_channel_kernel_features, expect=["conv"]),
    "conv tile 40 (bf16-split form)": _k(tk.test_conv_two_groups_tail_default_plan, kernel_path="bs0", expect=["conv"], env={"KG_CONV_BS": "1", "KG_CONV_BS_TILE": "0"}),
    "conv tile 41": _k(tk.test_conv_two_groups_tail_default_plan, kernel_path="bs1", expect=["conv"], env={"KG_CONV_BS": "1", "KG_CONV_BS_TILE": "1"}),
    "conv tile 42": _k(tk.test_conv_two_groups_tail_default_plan, kernel_path="bs2", expect=["conv"], env={"KG_CONV_BS": "1", "KG_CONV_BS_TILE": "2"}),
    "conv on packed weights": _k(tk.test_packed_weights_cached_across_launches, expect=["conv", "conv_pack"]),
    "conv general instantiation": _k(tk.test_conv_time_taps, 1, 5, 3, 7, 16, 3, 1, False, expect=["conv"], env={"KG_CONV_FAST": "0", "KG_CONV_TINY": "0"}),
    "conv N = 1, M = 3": _k(tk.test_conv_time_taps, 1, 5, 3, 7, 16, 3, 1, True, expect=["conv"]),
    "conv M = 2 rows, residual + mask": _k(tk.test_conv_few_rows_with_residual_and_mask, 2, expect=["conv"]),
    "conv M = 33 rows, residual + mask": _k(tk.test_conv_few_rows_with_residual_and_mask, 33, expect=["conv"]),
    "conv mask epilogue": _k(tk.test_conv_mask_epilogue, 2, 40, 70, 9, 7, 1, expect=["conv"]),
    "conv K-split: in-kernel completion and epilogue launch, tile 4 x 3": _k(tk.test_ksplit_completion_forms_are_deterministic, fast="0", tile=4, split=3, expect=["conv"]),
    "conv K-split: both completions, tile 9 x 2": _k(tk.test_ksplit_completion_forms_are_deterministic, fast="1", tile=9, split=2, expect=["conv"]),
    "conv K-split: both completions, tile 3 x 8": _k(tk.test_ksplit_completion_forms_are_deterministic, fast="1", tile=3, split=8, expect=["conv"]),
    "conv wave K-split, M 33, Cin 70": _k(tk.test_conv_wave_ksplit_tile, 33, 70, 6, 5, 3, False, expect=["conv"]),
    "conv wave K-split transposed, V = 1": _k(tk.test_conv_wave_ksplit_tile, 96, 80, 8, 1, 5, True, expect=["conv"]),
    "conv parity launches (o_tstride)": _k(tk.test_transposed_stride2_tcn_as_two_parity_launches, 2, 96, 8, 1, expect=["conv"]),
    "conv_many": _k(tk.test_conv_many_equals_single_launches, 64, 2, 6, kernel_path="default", expect=["conv_many"]),
    "conv V_out 70 through a vertex map (map entries loaded per column)": _k(tf.test_edge, "V_out 70 vmap forward", expect=["conv"]),
    "conv_many, an XCD-grouped job between two plain ones": _k(tf.test_many, "many three jobs one XCD", expect=["conv_many"]),
    "conv chanblock / blocked transpose, N = 1": _k(tk.test_conv_chanblock_and_blocked_transpose, 1, 7, 33, 5, 3, expect=["conv"]),
    "wgrad ragged": _k(tk.test_wgrad, 3, 70, 65, 10, 7, 3, TAP_TIME, 2, expect=["wgrad"]),
    "wgrad one element": _k(tk.test_wgrad, 1, 1, 1, 1, 1, 3, TAP_TIME, 1, expect=["wgrad"]),
    "wgrad V = 1": _k(tk.test_wgrad, 4, 512, 512, 8, 1, 3, TAP_TIME, 2, expect=["wgrad"]),
    "wgrad channel-block taps": _k(tk.test_wgrad, 3, 16, 16, 12, 2, 3, TAP_CHANBLOCK, 1, expect=["wgrad"]),
    "wgrad operand pairs": _k(tk.test_wgrad_operand_pairs, (3, 5), 70, 65, 10, 7, 3, TAP_TIME, 2, expect=["wgrad"]),
    "wgrad deferred reductions": _k(tk.test_wgrad_deferred_reductions, expect=["wgrad", "wgrad_reduce_many"]),
    "wgrad vertex gather": _k(tk.test_wgrad_with_vertex_gather, expect=["wgrad"]),
    "wgrad_many": _k(tk.test_wgrad_many_layers_one_call, expect=["wgrad_many"]),
    "wgrad_many, several launches": _k(tk.test_wgrad_many_more_layers_than_one_launch_holds, expect=["wgrad_many"]),
    "wgrad_many 128x128 tile, ragged rows and channels": _k(tw.test_big_tile_forced_at_small_column_counts, "forced 128x128: ragged 130x200, pairs", "fp32", expect=["wgrad_many"]),
    "wgrad_many bf16-split tiles": _k(tw.test_small_tiles_all_in_one_call, "bf16split", expect=["wgrad_many"]),
    "aggconv ragged (M 33, Cin 40)": _k(tk.test_aggconv_fused_gcn, "ntu", 3, False, 9, 40, 33, 8, 0, expect=["aggconv"]),
    "aggconv block 0 weights inside their parent": _k(tk.test_aggconv_fused_gcn, "h36m", 0, True, 3, 2, 32, 32, 10, expect=["aggconv"]),
    "aggconv_label": _k(td.test_aggconv_label_vs_definition, "h36m", 10, 2, 13, 64, expect=["aggconv_label"]),
    "aggconv_label ntu120": _k(td.test_aggconv_label_vs_definition, "ntu", 120, 3, 5, 256, expect=["aggconv_label"]),
    "label_bias_bwd two launches": _k(td.test_label_bias_bwd_two_launches, "ntu", 120, 7, 256, "random, five empty classes", expect=["label_bias_bwd"]),
    "label_bias kernels": _k(tk.test_label_bias_kernels, "ntu", 7, 120, 4, expect=["label_bias_fwd", "label_bias_bwd"]),
    "agg N = 1": _k(tk.test_agg_family, 1, 5, 3, 16, 7, 3, 1, expect=["agg_expand", "agg_reduce", "agg_outer"]),
    "agg ragged": _k(tk.test_agg_family, 5, 33, 13, 17, 2, 1, 1, expect=["agg_expand", "agg_reduce", "agg_outer"]),
    "agg one element": _k(tk.test_agg_family, 1, 1, 1, 1, 1, 3, 1, expect=["agg_expand", "agg_reduce", "agg_outer"]),
    "agg V = 1": _k(tk.test_agg_family, 2, 512, 8, 1, 1, 3, 1, expect=["agg_expand", "agg_reduce", "agg_outer"]),
    "agg rep 3": _k(tk.test_agg_family, 2, 40, 6, 7, 16, 1, 3, expect=["agg_expand", "agg_reduce", "agg_outer"]),
    "agg_reduce residual + mask epilogue": _k(tk.test_agg_reduce_residual_and_mask_epilogue, 5, 64, 32, 5, 11, 2, True, 3, "auto", expect=["agg_reduce"]),
    "agg_reduce on the matrix cores, ragged last tile, residual + mask epilogue": _k(ta.test_agg_case, "mfma reduce SUB3 V5 485 frames", expect=["agg_reduce"]),
    "aggconv forced 64-row tile with two k-groups (642)": _k(ta.test_aggconv_case, "tile 642 XE6 XA1 ADD1", expect=["aggconv"]),
    "agg_outer deferred sums": _k(tk.test_agg_outer_deferred_sums_one_launch, expect=["agg_outer", "agg_outer_finish"]),
    "gen_expand / fold / adj_finish, 3 channels": _k(tk.test_gen_expand_fold_adjfinish, *tk.GEN_CASES[0], expect=["gen_expand", "gen_fold", "gen_adj_finish"]),
    "gen_expand / fold / adj_finish, single vertex": _k(tk.test_gen_expand_fold_adjfinish, *tk.GEN_CASES[4], expect=["gen_expand", "gen_fold", "gen_adj_finish"]),
    "gen_expand / fold, no residual": _k(tk.test_gen_expand_fold_adjfinish, *tk.GEN_CASES[5], expect=["gen_expand", "gen_fold"]),
    "gen_expand / fold, residual alone": _k(tk.test_gen_expand_fold_adjfinish, *tk.GEN_CASES[6], expect=["gen_expand", "gen_fold"]),
    "gen_tail backward": _k(tk.test_gen_tail_backward_kernels, 64, 3, 64, 25, False, "identity", "tanh", expect=["gen_tail_bwd"]),
    "genblock fwd / bwd G3": _k(tk.test_genblock_fused_forward_backward, *tk.GENBLOCK_CASES[0], expect=["genblock_fwd", "genblock_bwd"]),
    "genblock fwd / bwd G5 (3 output channels)": _k(tk.test_genblock_fused_forward_backward, *tk.GENBLOCK_CASES[2], expect=["genblock_fwd", "genblock_bwd"]),
    "genblock fwd / bwd G6 (identity, tanh)": _k(tk.test_genblock_fused_forward_backward, *tk.GENBLOCK_CASES[3], expect=["genblock_fwd", "genblock_bwd"]),
    "genblock fwd / bwd h36m": _k(tk.test_genblock_fused_forward_backward, *tk.GENBLOCK_CASES[6], expect=["genblock_fwd", "genblock_bwd"]),
    "genblock fwd / bwd rep 3": _k(tk.test_genblock_fused_forward_backward, *tk.GENBLOCK_CASES[8], expect=["genblock_fwd", "genblock_bwd"]),
    "bn_fwd_many": _k(tk.test_bn_fwd_many_equals_per_group_launches, [(2, 3, 64, 25), (2, 70, 9, 7), (8, 5, 300, 3), (4, 1, 1, 1)], expect=["bn_fwd_many"]),
    "bn_bwd_many": _k(tk.test_bn_bwd_many_equals_single_launches, expect=["bn_bwd_many"]),
    "bn coefficients, one element": _k(tk.test_batchnorm_coefficients, 3, 1, 1, 1, True, expect=["bn_fwd", "bn_bwd"]),
    "bn coefficients, N = 1": _k(tk.test_batchnorm_coefficients, 1, 7, 5, 3, False, expect=["bn_fwd"]),
    "rowsum_many": _k(tk.test_rowsum_many_one_launch, expect=["rowsum_many"]),
    "rowsum product row": _k(tk.test_rowsum_product_row_alone, expect=["rowsum", "rowsum_many"]),
    "rowsum / affine_act / act_bwd, N = 1": _k(tk.test_rowsum_and_pointwise, 1, 7, 5, 3, expect=["rowsum", "affine_act", "act_bwd"]),
    "rowsum / pointwise, V = 1": _k(tk.test_rowsum_and_pointwise, 3, 256, 4, 1, expect=["rowsum"]),
    "rowsum destinations": _k(tk.test_rowsum_destinations, 1, 7, 5, 3, expect=["rowsum"]),
    "affine_act per-batch coefficients": _k(tk.test_affine_act_per_batch_coefficients, expect=["affine_act"]),
    "head_*": _k(tk.test_head_kernels, 5, 70, 3, 2, expect=["head_fwd", "head_bwd", "head_wgrad"]),
    "head_* V = 1": _k(tk.test_head_kernels, 64, 512, 2, 1, expect=["head_fwd", "head_bwd", "head_wgrad"]),
    "linear_* / embed_bwd ragged": _k(tk.test_mapping_network_kernels, 33, 37, 6, 5, expect=["linear_fwd", "linear_bwd", "embed_bwd"]),
    "linear_* without labels": _k(tk.test_mapping_network_kernels, 128, 96, 8, 0, expect=["linear_fwd", "linear_bwd"]),
    "gp_*": _k(tk.test_gradient_penalty_kernels, 3, 7, 9, 5, expect=["gp_fwd", "gp_bwd"]),
    "masked_adj_* / mix3": _k(tk.test_mix3_and_masked_adjacency_kernels, expect=["mix3", "masked_adj_fwd", "masked_adj_bwd"]),
    "adam_step*": _k(tk.test_adam_matches_torch, expect=["adam_step"]),
    "adam_step_ema, unaligned": _k(te.test_kernel_against_definition, 4101, 1, expect=["adam_step_ema"]),
    "sample_inputs": _k(ts.test_sample_inputs_against_definition, "ntu", 7, 512, expect=["sample_inputs"]),
    "trunc_lerp": _k(ts.test_trunc_lerp_against_definition, (3, 70, 33, 0.5, 3), expect=["trunc_lerp"]),
    "bn_eval_coef": _k(ts.test_bn_eval_coef_against_definition_and_live_statistics, expect=["bn_eval_coef"]),
    "step_inputs": _k(tt.test_kernel_against_definition, "TMP", "ntu", 5, 1, expect=["step_inputs"]),
    "step_inputs strided source": _k(tt.test_kernel_strided_source_and_random_only, "TMP", expect=["step_inputs"]),
}


def _body(case, tmp_path_factory, monkeypatch, golden_dir):
    fn, args, kw, _, env = case
    params = inspect.signature(fn).parameters

    def body():
        e = Env(monkeypatch)
        try:
            for k, v in env.items():
                e.setenv(k, v)
            a = [tmp_path_factory.mktemp("guarded") if x == "TMP" else x for x in args]
            k2 = dict(kw)
            if "monkeypatch" in params:
                k2["monkeypatch"] = e
            if "golden_dir" in params:
                k2["golden_dir"] = golden_dir
            fn(*a, **k2)
        finally:
            e.undo()
    return body


@pytest.mark.parametrize("name", list(KERNEL_CASES))
def test_kernel_results_do_not_depend_on_prior_memory(name, tmp_path_factory, monkeypatch, golden_dir):
    case = KERNEL_CASES[name]
    ab(_body(case, tmp_path_factory, monkeypatch, golden_dir), expect=case[3])


def test_every_family_is_covered():
    """(the cases above name the entry points they must launch; together they cover the binding's kernel families)"""
    covered = set()
    for case in KERNEL_CASES.values():
        covered |= set(case[3])
    missing = [n for n in ENTRY if n not in covered and n not in
               ("genblock_supported", "aggconv_supported", "gen_adj_prepare", "genblock_infer", "mmd", "loss_append")]
    assert not missing, missing          # (genblock_infer, mmd, loss_append: the cases further down; gen_adj_prepare: the generator steps)


@pytest.mark.parametrize("form", ["ct", "rt"])
def test_genblock_infer_does_not_depend_on_prior_memory(form, golden_dir, monkeypatch):
    ab(lambda: ts.test_genblock_infer_vs_reference_golden("ntu", form, golden_dir, Env(monkeypatch)), expect=["genblock_infer"])


def test_loss_append_writes_one_slot_only():
    """kg_loss_append into a ring the harness allocated: slot (step - 1) mod len and nothing else"""
    def body():
        ring = guard.full((5, 2), 7.0, device=DEV)
        step = guard.full((1,), 8, dtype=torch.int64, device=DEV)
        d, g = torch.tensor([1.5], device=DEV), torch.tensor([-2.5], device=DEV)
        nv.loss_append(ring, step, d, g)
        step += 1
        nv.loss_append(ring, step, d + 1, None)
        want = torch.full((5, 2), 7.0)
        want[2] = torch.tensor([1.5, -2.5])
        want[3, 0] = 2.5
        got = ring.cpu()
        assert torch.equal(got[:3], want[:3]) and got[3, 0] == 2.5 and torch.equal(got[4], want[4]), got
        return ring
    ab(body, expect=["loss_append"])


# ---- input side: operands between red zones ---------------------------------------------------------------------------------
INPUT_SIDE = {
    "conv M = 2": _k(tk.test_conv_few_rows_with_residual_and_mask, 2),
    "conv M = 3": _k(tk.test_conv_few_rows_with_residual_and_mask, 3),
    "conv M = 5": _k(tk.test_conv_few_rows_with_residual_and_mask, 5),
    "conv M = 33": _k(tk.test_conv_few_rows_with_residual_and_mask, 33),
    "conv 3 taps, every tile, lead 0": _k(tk.test_conv_forced_tiles_on_plane_tensors, 3, 17, 70, 9, 25, 3, TAP_TIME, False),
    "conv 3 taps transposed, V = 1": _k(tk.test_conv_forced_tiles_on_plane_tensors, 70, 40, 96, 64, 1, 3, TAP_TIME, True),
    "conv full slices (FAST), 3 taps": _k(tk.test_conv_time_taps, 2, 32, 64, 64, 11, 3, 1, False),
    "conv stride 2, V = 1": _k(tk.test_conv_time_taps, 4, 256, 512, 16, 1, 3, 2, False),
    "conv tiny-channel kernel": _k(tk.test_conv_tiny_channel_kernel_features),
    "conv bf16-split form, 16-byte window loads": _k(tk.test_conv_two_groups_tail_default_plan, kernel_path="bs0", env={"KG_CONV_BS": "1", "KG_CONV_BS_TILE": "0"}),
    "conv K-split, residual + mask": _k(tk.test_ksplit_completion_forms_are_deterministic, fast="1", tile=4, split=3),
    "conv wave K-split": _k(tk.test_conv_wave_ksplit_tile, 33, 70, 6, 5, 3, False),
    "conv V_out 70 through a vertex map": _k(tf.test_edge, "V_out 70 vmap transposed"),
    "aggconv ragged": _k(tk.test_aggconv_fused_gcn, "ntu", 3, False, 9, 40, 33, 8, 0),
    "aggconv block 0": _k(tk.test_aggconv_fused_gcn, "ntu", 0, True, 3, 3, 32, 64, 60),
    "wgrad ragged": _k(tk.test_wgrad, 3, 70, 65, 10, 7, 3, TAP_TIME, 2),
    "wgrad one element": _k(tk.test_wgrad, 1, 1, 1, 1, 1, 3, TAP_TIME, 1),
    "wgrad N = 5, V = 16": _k(tk.test_wgrad, 5, 33, 20, 9, 16, 3, TAP_TIME, 1),
    "wgrad channel-block taps": _k(tk.test_wgrad, 2, 63, 32, 64, 11, 3, TAP_CHANBLOCK, 1),
    "wgrad operand pairs": _k(tk.test_wgrad_operand_pairs, (3, 5), 70, 65, 10, 7, 3, TAP_TIME, 2),
    "wgrad vertex gather": _k(tk.test_wgrad_with_vertex_gather),
    "wgrad_many 128x128 tile, ragged rows and channels": _k(tw.test_big_tile_forced_at_small_column_counts, "forced 128x128: ragged 130x200, pairs", "fp32"),
    "wgrad_many 128x128 tile, 129x255": _k(tw.test_big_tile_forced_at_small_column_counts, "forced 128x128: ragged 129x255, 70 columns", "bf16split"),
    "wgrad_many bf16-split tiles": _k(tw.test_small_tiles_all_in_one_call, "bf16split"),
}


@pytest.mark.parametrize("name", list(INPUT_SIDE))
def test_guarded_operands_give_the_same_bits(name, tmp_path_factory, monkeypatch, golden_dir):
    """every load stays inside [base, base + extent) of its operand - or the value it fetched never reaches a result"""
    body = _body(INPUT_SIDE[name], tmp_path_factory, monkeypatch, golden_dir)
    plain, calls, _ = run_case(body, "A", outputs_only=True)
    guarded, _, g = run_case(body, "A", guard_operands=True, outputs_only=True)
    assert any(calls[n] for n in GUARDED_OPERANDS) and plain
    for what, _, _, bits in guarded:
        assert not (bits[:bits.numel() // 4 * 4].view(torch.int32) == PATTERN_A).any(), what + ": poison in a result"
    same_bits(plain, guarded, "plain operands", "operands between red zones")


# ---- model level ----------------------------------------------------------------------------------------------------------
REACHED = collections.Counter()          # (decision, arm) -> runs that took it, over the model-level cases of this module
DECISIONS = ("meta.any_single", "meta.sel is not None")


def _note_arms(g):
    for kind in ("zeros", "empty"):
        for line in g.source_lines(kind):
            for dec in DECISIONS:
                if dec in line and "torch.zeros" in line and "torch.empty" in line:
                    REACHED[(dec, kind)] += 1


def _shallow(D, c, nn0, k=4):
    """the critic's first k blocks with their own head: no single-vertex level, so TrunkMeta.any_single is False"""
    meta = D._trunk_meta(c["t_size"], nn0, torch.device(DEV))
    D.st_gcn_networks = torch.nn.ModuleList(list(D.st_gcn_networks)[:k])
    D.edge_importance = torch.nn.ParameterList(list(D.edge_importance)[:k])
    fcn = torch.nn.Linear(meta.geoms[k - 1].cout, 1)
    with torch.no_grad():
        fcn.weight.copy_(torch.linspace(-0.05, 0.05, fcn.weight.numel()).view_as(fcn.weight))
        fcn.bias.fill_(0.01)
    D.fcn = fcn.to(DEV)
    D._trunk_cache = {}
    assert D._trunk_meta(c["t_size"], nn0, torch.device(DEV)).any_single is False
    return D


def _trainer_step(cfg, n, shallow=False):
    def body():
        c, G, D, _, _ = build_pair(cfg, device=DEV)
        nn_ = G.graph.num_node
        if shallow:
            D = _shallow(D, c, nn_[0])
        real, labels, z, alpha = rand_inputs(n, c["channels"], c["t_size"], nn_[0], c["n_classes"], c["latent"], seed=3, device=DEV)
        nd, ng = rand_noise(n, c["t_size"], nn_, seed=6, device=DEV), rand_noise(n, c["t_size"], nn_, seed=7, device=DEV)
        tr = Trainer(G, D)
        out = []
        with tr.sharing_mapping(noise_g=ng):           # as Trainer.iteration: both syntheses next to the critic step
            out.append(tr.d_compute(real, labels, z, alpha, nd))
        out.append(tr.fD.grad.clone())                 # the critic's flat gradient bucket before the optimiser
        tr.d_apply()
        out.append(tr.g_compute(labels, z, ng))
        out.append(tr.fG.grad.clone())
        tr.g_apply()
        out += [tr.fD.flat, tr.fG.flat, tr.fD.exp_avg, tr.fD.exp_avg_sq, tr.fG.exp_avg, tr.fG.exp_avg_sq]
        out += [b for m in (G, D) for b in m.buffers()]
        for t in out[:4]:
            assert torch.isfinite(t).all()
        return out
    return body


@pytest.mark.parametrize("d0_fused", [True, False], ids=["d0fused", "d0composed"])
@pytest.mark.parametrize("gen_fused", [True, False], ids=["genfused", "genstaged"])
@pytest.mark.parametrize("cfg,n", [("ntu", 5), ("h36m", 3), ("ntu", 64)])
def test_training_step_does_not_depend_on_prior_memory(cfg, n, gen_fused, d0_fused, monkeypatch):
    """one eager critic step + one generator step of Trainer: losses, both gradient buckets before the optimiser, the
    parameters, the Adam moments and the BatchNorm buffers after it"""
    monkeypatch.setattr(gen_trunk, "FUSED", gen_fused)
    monkeypatch.setattr(disc_trunk, "D0_FUSED", d0_fused)
    g = ab(_trainer_step(cfg, n), expect=["conv", "wgrad_many", "adam_step", "masked_adj_fwd", "masked_adj_bwd", "mix3", "gp_fwd"],
           count_only=True)
    assert (g.calls["genblock_fwd"] > 0) == gen_fused and (g.calls["genblock_bwd"] > 0) == gen_fused, dict(g.calls)
    if n >= 64:          # (block 0's fused route needs >= 8192 columns)
        assert (g.calls["aggconv_label"] > 0) == d0_fused, dict(g.calls)
    _note_arms(g)


@pytest.mark.parametrize("cfg,n", [("ntu", 5), ("h36m", 3)])
def test_training_step_of_a_critic_without_single_vertex_level(cfg, n):
    """`(torch.zeros if meta.any_single else torch.empty)` of disc_trunk.bwd_pass / dbl_pass: the `empty` arm - every block
    writes its whole slice of the adjacency gradient"""
    _note_arms(ab(_trainer_step(cfg, n, shallow=True), expect=["conv", "adam_step", "masked_adj_bwd"], count_only=True))


@pytest.mark.parametrize("cfg,n", [("ntu", 5), ("h36m", 3)])
def test_plain_autograd_backward_does_not_depend_on_prior_memory(cfg, n):
    """no flat buckets, no parameter sinks: MaskedAdjacencyFn.backward allocates the importance gradient itself - cleared for
    the critic (`sel`: kept columns only), `torch.empty_like` for the generator (every element is written)"""
    def body():
        c, G, D, _, _ = build_pair(cfg, device=DEV)
        nn_ = G.graph.num_node
        real, labels, z, _ = rand_inputs(n, c["channels"], c["t_size"], nn_[0], c["n_classes"], c["latent"], seed=3, device=DEV)
        noise = rand_noise(n, c["t_size"], nn_, seed=6, device=DEV)
        fake = G(z, labels, noise=noise)
        (D(fake, labels).sum() + D(real, labels).sum()).backward()
        grads = [p.grad for m in (G, D) for p in m.parameters()]
        assert all(g is not None and torch.isfinite(g).all() for g in grads)
        return [fake] + grads
    _note_arms(ab(body, expect=["conv", "masked_adj_bwd"], count_only=True))


def test_both_arms_of_every_zero_or_empty_decision_were_reached():
    """(runs after the model-level cases above; with a -k selection of this file it only checks what ran)"""
    if sum(REACHED.values()) == 0:          # a -k selection without the model-level cases: nothing to check
        return
    for dec in DECISIONS:
        for arm in ("zeros", "empty"):
            assert REACHED[(dec, arm)] > 0, "no case reached the %s arm of the `%s` decision: %s" % (arm, dec, dict(REACHED))


# ---- generation and evaluation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trunc_mode", ["-", "w"], ids=["plain", "w-truncated"])
def test_sampler_round_does_not_depend_on_prior_memory(trunc_mode):
    """two eager rounds (the --no-graph form) of Sampler for ntu: images and latents"""
    def body():
        c, G, _, _, _ = build_pair("ntu", device=DEV)
        s = Sampler(G, qtd=1, seed=11, trunc=None if trunc_mode == "-" else 0.7, trunc_mode=trunc_mode, mean_size=200,
                    use_graph=False)
        out = []
        for _ in range(2):
            imgs, _, z = s.next()
            assert torch.isfinite(imgs).all() and imgs.shape[0] == c["n_classes"]
            out += [imgs.clone(), z.clone()]
        return out
    ab(body, expect=["sample_inputs", "genblock_infer", "bn_eval_coef", "linear_fwd"] + (["trunc_lerp"] if trunc_mode == "w" else []))


@pytest.mark.parametrize("name", ["h36m", "ntu"])
@pytest.mark.parametrize("mode", ["avg", "joint"])
def test_calculate_mmd_does_not_depend_on_prior_memory(name, mode, golden_dir):
    """metrics.calculate_mmd on the inputs of tests/golden/mmd_ref.npz"""
    from tests import test_mmd_gpu as tm
    fake, real, lab, _ = tm._fixture(golden_dir, name)

    def body():
        mean, result, per_bw = metrics.calculate_mmd(torch.tensor(fake).cuda(), torch.tensor(real).cuda(), lab, mode, per_class=True)
        return [mean, result, per_bw]
    ab(body, expect=["mmd"])
