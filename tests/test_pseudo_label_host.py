"""Host side of the device-resident pseudo-labelling (zs3_pl_candidates / zs3_pl_select, zs3_amd/self_training.py): what needs no
GPU -- the entry points' place in the C ABI, the argument checks of the ops, the class masks and the keep-count formula."""
import ctypes
import math
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_exported_and_wrapped():
    from zs3_amd import build
    sigs = {name: (ret, params) for ret, name, params in build.parse_header()}
    for name in ("zs3_pl_ws_bytes", "zs3_pl_candidates", "zs3_pl_select"):
        assert name in sigs
    assert sigs["zs3_pl_ws_bytes"] == ("long", [("int", "N"), ("int", "C")])
    cand, sel = sigs["zs3_pl_candidates"][1], sigs["zs3_pl_select"][1]
    assert [n for _, n in cand] == ["scores", "ld", "N", "H", "W", "C", "target", "target_is_i64", "Ho", "Wo", "cand_lo", "cand_hi",
                                    "unl_lo", "unl_hi", "unlabelled_value", "ignore_index", "cls_map", "conf_map", "count", "stream"]
    assert [n for _, n in sel] == ["conf_map", "cls_map", "target", "target_is_i64", "N", "Ho", "Wo", "C", "cand_lo", "cand_hi",
                                   "count", "top_percent", "group", "ignore_index", "labels", "selected", "threshold", "totals", "ws",
                                   "stream"]
    # launching entry points on fp32 scores (no `io`), built from parameter types the wrapper generator already knows
    known = {"int", "long", "double", "unsigned long long"}
    for params in (cand, sel):
        assert params[-1] == ("void*", "stream") and ("int", "io") not in params
        assert all("*" in t or t in known for t, _ in params)
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in ("zs3_pl_ws_bytes", "zs3_pl_candidates", "zs3_pl_select"):
        assert hasattr(lib, name)
    rename = open(os.path.join(build.GEN, "plan_rename.h")).read()
    wrappers = open(os.path.join(build.GEN, "plan_wrappers.hip")).read()
    for name in ("zs3_pl_candidates", "zs3_pl_select"):
        assert f"#define {name} {name}__impl" in rename
        assert f'extern "C" int {name}(' in wrappers and f'{{"{name}", ' in wrappers
    assert "zs3_pl_ws_bytes" not in rename                 # not a launch: nothing to record


def test_lib_derives_the_argtypes_and_the_entry_points_check_their_arguments():
    from zs3_amd._lib import lib as bound
    L = bound()
    vp, i, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_ulonglong
    assert L.zs3_pl_ws_bytes.argtypes == [i, i] and L.zs3_pl_ws_bytes.restype is ctypes.c_long
    assert L.zs3_pl_candidates.argtypes == [vp, i, i, i, i, i, vp, i, i, i, u64, u64, u64, u64, i, i, vp, vp, vp, vp]
    assert L.zs3_pl_select.argtypes == [vp, vp, vp, i, i, i, i, i, u64, u64, vp, ctypes.c_double, i, i, vp, vp, vp, vp, vp, vp]
    assert {"zs3_pl_ws_bytes", "zs3_pl_candidates", "zs3_pl_select"} <= L._zs3_declared
    # the workspace: a 256-bin histogram, a prefix and a rank of 4 bytes each per (image, class); grows with both
    assert L.zs3_pl_ws_bytes(16, 21) >= 16 * 21 * 258 * 4 and L.zs3_pl_ws_bytes(16, 60) > L.zs3_pl_ws_bytes(16, 21)
    assert L.zs3_pl_ws_bytes(0, 21) < 0 and L.zs3_pl_ws_bytes(1, 129) < 0 and L.zs3_pl_ws_bytes(1, 0) < 0
    # argument validation happens before any launch (no GPU here: a launch would fail differently)
    for n, c in ((1, 0), (1, 129), (0, 21)):
        assert L.zs3_pl_candidates(None, c, n, 5, 5, c, None, 0, 9, 9, 1, 0, 1, 0, -1, 255, None, None, None, None) == -1
        assert L.zs3_pl_select(None, None, None, 0, n, 9, 9, c, 1, 0, None, 25.0, 0, 255, None, None, None, None, None, None) == -1


def test_ops_refuse_bad_arguments_before_touching_a_device():
    from zs3_amd import ops
    from zs3_amd._lib import Zs3HipError
    scores, target = torch.randn(2, 5, 5, 21), torch.zeros(2, 9, 9)
    cls_map, conf_map = torch.zeros(2, 9, 9, dtype=torch.uint8), torch.zeros(2, 9, 9)
    count = torch.zeros(2, 21, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.pl_candidates(scores.double(), target, [10, 14])
    with pytest.raises(TypeError):
        ops.pl_candidates(scores, target.int(), [10, 14])
    with pytest.raises(ValueError):
        ops.pl_candidates(scores, target[0], [10, 14])                        # not [N, H, W]
    with pytest.raises(ValueError):
        ops.pl_candidates(scores, torch.zeros(3, 9, 9), [10, 14])             # another batch size
    with pytest.raises(ValueError):
        ops.pl_candidates(scores[0], target, [10, 14])
    with pytest.raises(ValueError):
        ops.pl_candidates(torch.randn(1, 3, 3, 129), torch.zeros(1, 9, 9), [10])     # C > 128
    for bad in ([], [21], [-1]):
        with pytest.raises(ValueError):
            ops.pl_candidates(scores, target, bad)
    with pytest.raises(ValueError):
        ops.pl_candidates(scores, target, [10], unlabelled=[128])
    with pytest.raises(ValueError):
        ops.pl_candidates(scores, target, [10], cls_map=cls_map.float())
    for p in (-0.5, 100.5, float("nan")):
        with pytest.raises(ValueError):
            ops.pl_select(cls_map, conf_map, count, target, [10, 14], p)
        with pytest.raises(ValueError):
            ops.pseudo_label(scores, target, [10, 14], p)
    with pytest.raises(ValueError):
        ops.pl_select(cls_map, conf_map, count, target, [10, 14], 25.0, group="class")
    with pytest.raises(ValueError):
        ops.pseudo_label(scores, target, [10, 14], 25.0, group="per_image")
    with pytest.raises(ValueError):
        ops.pl_select(cls_map.int(), conf_map, count, target, [10, 14], 25.0)
    with pytest.raises(ValueError):
        ops.pl_select(cls_map, conf_map.double(), count, target, [10, 14], 25.0)
    with pytest.raises(ValueError):
        ops.pl_select(cls_map, conf_map, count.long(), target, [10, 14], 25.0)
    with pytest.raises(ValueError):
        ops.pl_select(cls_map, conf_map, torch.zeros(2, 129, dtype=torch.int32), target, [10, 14], 25.0)
    with pytest.raises(ValueError):
        ops.pl_select(cls_map, conf_map, count, target, [10, 14], 25.0, labels=torch.zeros(2, 9, 9, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.pl_select(cls_map, conf_map, count, target, [10, 14], 25.0, totals=torch.zeros(2, 21))
    with pytest.raises(ValueError):
        ops.pl_select(cls_map, conf_map, count, target, [10, 14], 25.0, ws=torch.zeros(16, dtype=torch.int32))
    # well-formed arguments on the CPU: refused, there is no fallback
    with pytest.raises(Zs3HipError):
        ops.pl_candidates(scores, target, [10, 14])
    with pytest.raises(Zs3HipError):
        ops.pl_select(cls_map, conf_map, count, target, [10, 14], 25.0)
    with pytest.raises(Zs3HipError):
        ops.pseudo_label(scores, target, [10, 14], 25.0, group="image")


def test_step_checks_its_arguments_and_has_no_cpu_fallback():
    from zs3_amd._lib import Zs3HipError
    from zs3_amd.modeling.deeplab import DeepLab
    from zs3_amd.self_training import PseudoLabelStep, pseudo_label_loader
    torch.manual_seed(0)
    model = DeepLab(num_classes=21, pretrained=False, sync_bn=False).eval()
    with pytest.raises(ValueError):
        PseudoLabelStep(model, [10, 14], group="pixel")
    with pytest.raises(ValueError):
        PseudoLabelStep(model, [10, 14], top_percent=120.0)
    with pytest.raises(ValueError):
        PseudoLabelStep(model, [])
    step = PseudoLabelStep(torch.nn.DataParallel(model), [14, 10, 14])
    assert step.model is model and step.candidates == [10, 14] and step.last_stats is None
    image, target = torch.randn(1, 3, 33, 33), torch.zeros(1, 33, 33)
    with pytest.raises(Zs3HipError):
        step.step(image, target)
    assert step.batches == 0


def test_class_mask():
    from zs3_amd.ops import class_mask
    assert class_mask([]) == (0, 0)
    assert class_mask([0]) == (1, 0) and class_mask([63]) == (1 << 63, 0)
    assert class_mask([64]) == (0, 1) and class_mask([127]) == (0, 1 << 63)
    assert class_mask([10, 14]) == ((1 << 10) | (1 << 14), 0)
    assert class_mask([14, 10, 14]) == class_mask((10, 14))                           # a set: order and repeats do not matter
    assert class_mask([3, 70, 64, 63]) == ((1 << 3) | (1 << 63), (1 << 6) | 1)
    assert class_mask(range(128)) == (2 ** 64 - 1, 2 ** 64 - 1)
    assert class_mask(torch.tensor([5, 100])) == (1 << 5, 1 << 36)
    for bad in ([128], [-1], [255]):
        with pytest.raises(ValueError):
            class_mask(bad)


def test_pl_keep_count():
    from zs3_amd.ops import pl_keep_count
    table = {  # (m, p) -> k = min(m, ceil(m * p / 100))
        (0, 0): 0, (0, 25): 0, (0, 100): 0,
        (1, 0): 0, (1, 12.5): 1, (1, 25): 1, (1, 75): 1, (1, 100): 1,
        (7, 0): 0, (7, 12.5): 1, (7, 25): 2, (7, 75): 6, (7, 100): 7,
        (8, 12.5): 1, (8, 25): 2, (8, 75): 6, (8, 100): 8,                            # m * p / 100 integral: no rounding up
        (200, 12.5): 25, (200, 25): 50, (200, 75): 150,
        (9, 12.5): 2, (101, 25): 26, (263169, 25): 65793, (263169, 75): 197377, (263169, 100): 263169,
    }
    for (m, p), k in table.items():
        assert pl_keep_count(m, p) == k, (m, p)
        assert pl_keep_count(m, p) == min(m, math.ceil(m * p / 100))
    for m in (1, 3, 1000):
        assert pl_keep_count(m, 1e-9) == 1                                            # any p > 0 keeps at least one pixel
