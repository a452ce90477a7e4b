"""The attention families where a gather offset passes 2 GiB: the layout, the configurations and the conditions on the inputs shared by
tests/test_attention_address_host.py and tests/test_gpu_attention_address_edges.py.

Every attention kernel reads its gathered operand through one buffer descriptor with a raw 32-bit byte offset, id * pitch_bytes, and the
families' domain functions (cabi.*_serves) admit rows * pitch * elem <= DENSE_BYTES_MAX = 3.5 GiB.  The domains put no cap on the pitch
itself, so the 200-row cases every attention test uses reach the far end of that domain as row-strided views of one large buffer:

    limit_pitch(200, 4) = DENSE_BYTES_MAX // 800       = 4,697,620 floats
    limit_pitch(200, 2) = DENSE_BYTES_MAX // 400, even = 9,395,240 16-bit elements
    first_far_row       = 115: rows 115..199 start at or past 2^31 bytes; the extent (199 pitch + k) elem is about 3.74e9 bytes

A larger pitch leaves the domain and fewer rows need a larger pitch, so these are the smallest shapes that set bit 31 in the offset, in
the descriptor's extent and in the load's offset argument.  `pitched` allocates exactly the extent such a view owns and fills ALL of it
with NaN before the rows are copied in: what lies between the rows is a trap for a gather that leaves its row, and the exact size one for
a descriptor whose extent is rows * pitch.

No case, reference or bound is made here: CONFIGS names, per kernel form, the cases of the families' own *_cases.py modules (one per
width instantiation, from constants those modules already have), with their own seeds, thresholds and a_edge.
"""
import numpy as np
import torch

from tests import attention16_cases
from tests import attention_cases
from tests import gat16_cases
from tests import gat_cases
from tests import gat_dropout_cases
from tests import gat_edge_cases
from tests import gatv2_16_cases
from tests import gatv2_cases
from tests import gatv2_dropout_cases
from tests import mha16_cases
from tests import mha_cases
from tests import mha_dropout_cases
from tests import rect_cases

FAR = 1 << 31
BF, FP = torch.bfloat16, torch.float16
ROWS = attention_cases.N                                    # both sides of the shared graph

WIDTH_CONFIGS = gat_dropout_cases.WIDTH_CONFIGS             # one per width instantiation of the head families: LPR 8, 16, 32, 64, 64 x 2
FORM_CONFIGS = ((1, 47), (8, 8), (1, 512))                  # the EDGE / DROP instantiations: one head, heads inside a chunk, two chunks
ATTENTION_WIDTHS = rect_cases.ATTENTION_WIDTHS + (512,)
ATTENTION16_SPECS = tuple((k, dtype) for k in rect_cases.ATTENTION16_WIDTHS for dtype in (BF, FP))
GAT16_SPECS = rect_cases.GAT16_SPECS
assert WIDTH_CONFIGS == gatv2_dropout_cases.WIDTH_CONFIGS == mha_dropout_cases.WIDTH_CONFIGS
assert set(FORM_CONFIGS) <= set(gat_cases.CONFIGS) and set(FORM_CONFIGS) <= set(gat_dropout_cases.EDGE_CONFIGS)

# form -> (kind: whose operands and entries, bytes per element, configurations, the case of one configuration)
CONFIGS = {
    "attention": ("attention", 4, tuple((k,) for k in ATTENTION_WIDTHS), attention_cases.width_case),
    "attention16": ("attention", 2, ATTENTION16_SPECS, attention16_cases.width_case),
    "gat": ("gat", 4, WIDTH_CONFIGS, gat_cases.config_case),
    "gat_edge": ("gat", 4, FORM_CONFIGS, gat_edge_cases.config_case),
    "gat_drop": ("gat", 4, FORM_CONFIGS, gat_dropout_cases.config_case),
    "gat_drop_edge": ("gat", 4, FORM_CONFIGS, gat_dropout_cases.edge_case),
    "gat16": ("gat", 2, GAT16_SPECS, gat16_cases.config_case),
    "gatv2": ("gatv2", 4, WIDTH_CONFIGS, gatv2_cases.config_case),
    "gatv2_drop": ("gatv2", 4, FORM_CONFIGS, gatv2_dropout_cases.config_case),
    "gatv2_16": ("gatv2", 2, GAT16_SPECS, gatv2_16_cases.config_case),
    "mha": ("mha", 4, WIDTH_CONFIGS, mha_cases.config_case),
    "mha_drop": ("mha", 4, FORM_CONFIGS, mha_dropout_cases.config_case),
    "mha16": ("mha", 2, GAT16_SPECS, mha16_cases.config_case),
}


def _layer_config(kind, elem):
    shape = (128,) if kind == "attention" else (8, 8)
    return shape + ((BF,) if elem == 2 else ())


# the one configuration per form that also goes through the operators and the plug-in: width 128, or (H, d) = (8, 8); 16 bits: bf16
LAYER_CONFIG = {form: _layer_config(kind, elem) for form, (kind, elem, _, _) in CONFIGS.items()}


def config_id(config):
    return "-".join(attention16_cases.dtype_name(v) if isinstance(v, torch.dtype) else str(v) for v in config)


def all_configs():
    """[(form, config)] of every kernel form at every configuration."""
    return [(form, config) for form, (_, _, configs, _) in CONFIGS.items() for config in configs]


def ids(pairs):
    return [f"{form}-{config_id(config)}" for form, config in pairs]


def kind_of(form):
    return CONFIGS[form][0]


def elem_bytes(form):
    return CONFIGS[form][1]


def case_of(form, config):
    return CONFIGS[form][3](*config)


def _serves(rows, pitch, elem):
    """Every family's own domain function of isplib_amd.cabi, at its narrowest admitted width, on `rows` gathered rows at `pitch`."""
    from isplib_amd import cabi
    if elem == 4:
        return (cabi.attention_serves(rows, 1, pitch), cabi.gat_serves(rows, 1, 1, pitch), cabi.gatv2_serves(rows, 1, 1, pitch),
                cabi.mha_serves(rows, 1, 1, pitch))
    return (cabi.attention16_serves(rows, 8, pitch), cabi.gat16_serves(rows, 1, 8, pitch), cabi.gatv2_16_serves(rows, 1, 8, pitch),
            cabi.mha16_serves(rows, 1, 8, pitch))


def limit_pitch(rows, elem):
    """The largest pitch (in elements; even for the 2-byte families) the families' own *_serves admit for `rows` gathered rows."""
    from isplib_amd import cabi
    assert elem in (2, 4) and rows > 0
    step = 1 if elem == 4 else 2
    pitch = cabi.DENSE_BYTES_MAX // (elem * rows) // step * step
    assert all(_serves(rows, pitch, elem)), (rows, pitch)
    assert not any(_serves(rows, pitch + step, elem)), (rows, pitch + step)
    return pitch


def first_far_row(pitch, elem):
    """The first row whose byte offset row * pitch * elem is at or past 2^31."""
    return -(-FAR // (pitch * elem))


def extent(rows, k, pitch):
    """Elements a row-strided view [rows, k] at `pitch` owns."""
    return (rows - 1) * pitch + k


def assert_reaches(case, pitch, elem):
    """A condition on the INPUTS: the case's graph sends gathers to both sides of 2^31 bytes in both walks.  In the CSR walk (forward, rows
    backward) the gathered row is an entry's column: the first row, far - 1, far and the last row are each referenced, and the hub column
    lies at or past far.  In the transposed walk (columns backward) the gathered row is the entry's row: far - 1, far and the last row
    have entries, and so has a row below them (row 0 itself is the shared graph's empty row, on purpose: LENGTHS[0] == 0).  Returns far."""
    rowptr, col = np.asarray(case.rowptr), np.asarray(case.col)
    m, far = rowptr.size - 1, first_far_row(pitch, elem)
    indeg, deg = np.bincount(col, minlength=0), np.diff(rowptr)
    n = indeg.size
    assert 1 < far < min(m, n), (far, m, n)
    for j in (0, far - 1, far, n - 1):
        assert indeg[j] > 0, f"no entry gathers row {j} of the column side"
    assert int(np.argmax(indeg)) >= far and indeg.max() >= 1000, "the hub column lies below 2^31 bytes"
    for i in (far - 1, far, m - 1):
        assert deg[i] > 0, f"row {i} is empty: the columns backward never gathers it"
    assert deg[:far - 1].any() and (deg[far:] > 0).sum() > 50 and (col >= far).mean() > 0.4
    return far


def pitched_out(rows, k, pitch, dtype, device, fill=float("nan")):
    """-> a view [rows, k] at `pitch` of a fresh buffer of exactly extent(rows, k, pitch) elements, every one of them `fill`."""
    assert pitch >= k and rows > 0
    buf = torch.full((extent(rows, k, pitch),), fill, dtype=dtype, device=device)
    return buf.as_strided((rows, k), (pitch, 1))


def pitched(t, pitch, fill=float("nan")):
    """`t` [rows, k] as a view at `pitch` of a buffer of exactly the extent that view owns, `fill` everywhere between the rows."""
    view = pitched_out(t.size(0), t.size(1), pitch, t.dtype, t.device, fill)
    view.copy_(t)
    return view


def buffer_of(view):
    """The whole buffer behind a view made by pitched / pitched_out."""
    base = view._base
    assert base is not None and base.dim() == 1 and base.numel() == extent(view.size(0), view.size(1), view.stride(0))
    return base


def pads_keep_nan(view):
    """Every element of the view was written (none is NaN) and every element between the rows still is NaN."""
    assert not torch.isnan(view).any(), "an element of the output was not written"
    assert int(torch.isnan(buffer_of(view)).sum()) == buffer_of(view).numel() - view.numel(), "written between the rows"
