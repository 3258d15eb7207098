"""CPU: every refusal of the five dg_adamw_step* entries and the two dg_grad_norm_finalize* entries, with made-up non-NULL addresses.
Each call below is wrong in at least one way, so the library returns before it launches anything: nothing here needs a GPU, and
nothing here may be turned into a valid call (a valid call would launch on those addresses)."""
import pytest

ARG, ALIGN = -1, -2
# the argument lists of include/drakegpt_hip.h, in order; every entry ends in the stream
PREFIX = ("p", "g", "m", "v", "n", "hyper", "rng_state", "grad_scale")
SCHED = ("clip_coef", "lr_table", "lr_table_len", "no_decay_bits", "shadow", "advance")
ENTRIES = {
    "dg_adamw_step": PREFIX + ("shadow", "advance"),
    "dg_adamw_step_clip": PREFIX + ("clip_coef", "shadow", "advance"),
    "dg_adamw_step_sched": PREFIX + SCHED,
    "dg_adamw_step_ema": PREFIX + SCHED + ("ema", "ema_hyper"),
    "dg_adamw_step_guard": PREFIX + SCHED + ("ema", "ema_hyper", "guard", "data_state"),
}
# a call that would be accepted (and is therefore never made): 16-byte aligned addresses, all distinct
VALID = dict(p=0x10000, g=0x20000, m=0x30000, v=0x40000, n=1027, hyper=0x50000, rng_state=0x60000, grad_scale=0.5, clip_coef=0x70000,
             lr_table=0x80000, lr_table_len=3, no_decay_bits=0x90000, shadow=0xA0000, advance=1, ema=0xB0000, ema_hyper=0xC0000,
             guard=0xD0000, data_state=0xE0000)
REQUIRED = {
    "dg_adamw_step": ("p", "g", "m", "v", "hyper", "rng_state"),
    "dg_adamw_step_clip": ("p", "g", "m", "v", "hyper", "rng_state", "clip_coef"),
    "dg_adamw_step_sched": ("p", "g", "m", "v", "hyper", "rng_state"),
    "dg_adamw_step_ema": ("p", "g", "m", "v", "hyper", "rng_state", "ema", "ema_hyper"),
    "dg_adamw_step_guard": ("p", "g", "m", "v", "hyper", "rng_state", "guard"),
}
STREAMS = {name: ("p", "g", "m", "v") + (("ema",) if "ema" in args else ()) for name, args in ENTRIES.items()}
TABLE_MISMATCHES = ((None, 1), (None, -1), (0x80000, 0), (0x80000, -2))
WITH_TABLE = [name for name, args in ENTRIES.items() if "lr_table" in args]


def _refused(entry, **wrong):
    """the entry's return code for VALID with `wrong` laid over it; at least one of the overrides must make the call a refused one"""
    from drakegpt_amd import _lib
    assert wrong and set(wrong) <= set(ENTRIES[entry]), (entry, wrong)
    args = dict(VALID, **wrong)
    return getattr(_lib.lib, entry)(*[args[a] for a in ENTRIES[entry]], None)


def test_the_entries_are_bound_with_these_argument_lists():
    from drakegpt_amd import _lib
    for entry, args in ENTRIES.items():
        assert hasattr(_lib.lib, entry) and len(_lib.SIGNATURES[entry]) == len(args) + 1, entry
    assert _lib.lib.dg_version() == 21


@pytest.mark.parametrize("entry", ENTRIES)
def test_null_pointers_and_empty_sizes(entry):
    for name in REQUIRED[entry]:
        assert _refused(entry, **{name: None}) == ARG, (entry, name)
    for n in (0, -4):
        assert _refused(entry, n=n) == ARG, (entry, n)


@pytest.mark.parametrize("entry", ENTRIES)
def test_misaligned_streams(entry):
    for name in STREAMS[entry]:
        for off in (4, 8, 12):
            assert _refused(entry, **{name: VALID[name] + off}) == ALIGN, (entry, name, off)


@pytest.mark.parametrize("entry", WITH_TABLE)
def test_lr_table_and_its_length_go_together(entry):
    for table, length in TABLE_MISMATCHES:
        assert _refused(entry, lr_table=table, lr_table_len=length) == ARG, (entry, table, length)


def test_guard_entry_pairs_and_aliases():
    assert _refused("dg_adamw_step_guard", ema=None) == ARG                       # ema_hyper alone
    assert _refused("dg_adamw_step_guard", ema_hyper=None) == ARG                 # ema alone
    assert _refused("dg_adamw_step_guard", data_state=VALID["rng_state"]) == ARG
    # a misaligned ema is looked at only where there is one to look at; with a second defect the call is still a refused one
    assert _refused("dg_adamw_step_guard", ema=VALID["ema"] + 4, ema_hyper=None) == ARG


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_come_before_alignment_errors(entry):
    bent = {"p": VALID["p"] + 4, "v": VALID["v"] + 4}
    assert _refused(entry, **bent) == ALIGN
    for name in REQUIRED[entry]:
        if name not in bent:
            assert _refused(entry, **bent, **{name: None}) == ARG, (entry, name)
    assert _refused(entry, **bent, n=0) == ARG
    if entry in WITH_TABLE:
        for table, length in TABLE_MISMATCHES:
            assert _refused(entry, **bent, lr_table=table, lr_table_len=length) == ARG, (entry, table, length)
    if "ema" in ENTRIES[entry]:
        assert _refused(entry, ema=VALID["ema"] + 4, hyper=None) == ARG
    if entry == "dg_adamw_step_guard":
        assert _refused(entry, **bent, ema=None) == ARG
        assert _refused(entry, **bent, ema_hyper=None) == ARG
        assert _refused(entry, **bent, data_state=VALID["rng_state"]) == ARG


def test_finalize_entries():
    from drakegpt_amd import _lib
    lib = _lib.lib
    part, max_norm, out, limit, loss, guard = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    for bad in ((None, 4, 1.0, max_norm, out), (part, 4, 1.0, None, out), (part, 4, 1.0, max_norm, None), (part, 0, 1.0, max_norm, out),
                (part, -3, 1.0, max_norm, out), (None, 0, 1.0, None, None)):
        assert lib.dg_grad_norm_finalize(*bad, None) == ARG, bad
    for bad in ((None, 4, 1.0, max_norm, out, limit, loss, guard), (part, 4, 1.0, max_norm, None, limit, loss, guard),
                (part, 4, 1.0, max_norm, out, None, loss, guard), (part, 4, 1.0, max_norm, out, limit, loss, None),
                (part, 0, 1.0, max_norm, out, limit, loss, guard), (part, -3, 1.0, max_norm, out, limit, loss, guard),
                (part, 4, 1.0, None, out, limit, None, None)):          # the two optional operands absent, and no guard
        assert lib.dg_grad_norm_finalize_guard(*bad, None) == ARG, bad
