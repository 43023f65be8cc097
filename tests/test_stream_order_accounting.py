"""Every prototype of include/beast_hip.h that takes a stream is accounted for by the seven
stream-order modules.  Needs no GPU: importing the modules registers their cases and touches no
device, and the rest is the header."""
import re

import stream_order as SO
import test_gpu_blend_stream_order
import test_gpu_logits_stream_order
import test_gpu_sample_stream_order
import test_gpu_score_stream_order
import test_gpu_stream_order
import test_gpu_windows_stream_order
import test_gpu_xent_stream_order
from test_lib_exports import header_protos

MODULES = [test_gpu_stream_order, test_gpu_logits_stream_order, test_gpu_xent_stream_order,
           test_gpu_sample_stream_order, test_gpu_score_stream_order, test_gpu_windows_stream_order,
           test_gpu_blend_stream_order]
GROUPS = ("PROBED", "SYNCHRONOUS", "NOT_PROBED", "NO_LAUNCH")     # a module defines those it needs


def test_every_stream_export_is_accounted_for():
    """Every prototype with a ``void*`` parameter whose name contains ``stream`` spells it ``stream``,
    is in exactly one group of exactly one module, has a section-A case there if the group is probed,
    and is named in that module's docstring: a new entry point cannot dodge the probe, whatever it
    calls its parameter."""
    spelled = {name: re.findall(r"void\s*\*\s*(\w*stream\w*)", args, flags=re.I)
               for name, args in header_protos().items()}
    takes_stream = {name for name, params in spelled.items() if params}
    assert len(takes_stream) >= 40, "the header parse found too few prototypes that take a stream"
    assert all(spelled[name] == ["stream"] for name in takes_stream), \
        {name: spelled[name] for name in takes_stream if spelled[name] != ["stream"]}

    listed = [(name, mod, group) for mod in MODULES for group in GROUPS for name in getattr(mod, group, ())]
    names = [name for name, _, _ in listed]
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)
    assert set(names) == takes_stream, (sorted(takes_stream - set(names)), sorted(set(names) - takes_stream))
    for name, mod, group in listed:
        assert re.search(rf"\b{name}\b", mod.__doc__), f"{name} is missing from the docstring of {mod.__name__}"
        if group not in ("PROBED", "SYNCHRONOUS"):
            assert getattr(mod, group)[name], f"{name}: {group} without a reason"
    assert all(n.startswith("beast_comm_") or n == "beast_bpe_train_comm"
               for mod in MODULES for n in getattr(mod, "NOT_PROBED", ()))

    for mod in MODULES:
        probed = set(getattr(mod, "PROBED", ())) | set(getattr(mod, "SYNCHRONOUS", ()))
        covered = {e for module, entries, _ in SO.CASES.values() if module == mod.__name__ for e in entries}
        assert covered == probed, (mod.__name__, sorted(probed - covered), sorted(covered - probed))
    assert {module for module, _, _ in SO.CASES.values()} <= {mod.__name__ for mod in MODULES}
