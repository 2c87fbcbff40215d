"""Bookkeeping shared by the kernel-against-fp64 tests (test_gpu_loss_kernels.py, test_gpu_body_kernels.py): the worst
error of a kernel per quantity, checked against a gate that never comes from the code under test, and one printed line per
quantity under ``-s``."""
import torch

U24, U8 = 2.0 ** -24, 2.0 ** -8


class Worst:
    """Worst error of the kernel per quantity over the inner cases of one test, with torch-fp32's error and the gate of
    that same inner case; report() prints one line per quantity, each beginning with ``prefix``."""

    def __init__(self, tag, prefix="loss-kernel-errors:"):
        self.tag, self.prefix, self.rows, self._ratio = tag, prefix, {}, {}

    def check(self, what, got, want, ref32, floor, bf16_out=False, relative=False, where=""):
        """got: the kernel's result; want: fp64; ref32: torch's fp32 composition; floor: the kernel's earlier gate as a
        multiple of max(1, |want|max) (relative: of |want|max)."""
        got, want, ref32 = got.detach().double().cpu(), want.detach().double().cpu(), ref32.detach().double().cpu()
        assert got.shape == want.shape == ref32.shape, (what, got.shape, want.shape, ref32.shape)
        top = float(want.abs().max()) if want.numel() else 0.0
        e32 = float((ref32 - want).abs().max()) if want.numel() else 0.0
        gate = max(floor * (top if relative else max(1.0, top)), 4.0 * e32)
        err = (got - want).abs()
        allow = gate + (U8 * want.abs() if bf16_out else 0.0)
        worst = float(err.max()) if want.numel() else 0.0
        row = self.rows.get(what)
        if row is None or worst > row[0]:
            self.rows[what] = (worst, e32, gate, where)
        assert bool((err <= allow).all()), (self.tag, what, where, "kernel", worst, "torch-fp32", e32, "gate", gate,
                                            "+ 2^-8 |want|" if bf16_out else "")

    def bound(self, what, got, want, allow, where="", e32=None):
        """Elementwise |got - want| <= allow (a tensor of want's shape, or a number).  Keeps the element nearest its bound:
        its error, its bound, and e32 (a tensor: the error of an fp32 restatement at that element) where one is given."""
        got, want = got.detach().double().cpu(), want.detach().double().cpu()
        assert got.shape == want.shape, (what, got.shape, want.shape)
        if not want.numel():
            return
        allow = allow.detach().double().cpu() if torch.is_tensor(allow) else torch.full_like(want, float(allow))
        err = (got - want).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / allow.clamp_min(1e-300)).reshape(-1)
        k = int(ratio.argmax())
        if what not in self._ratio or float(ratio[k]) > self._ratio[what]:
            self._ratio[what] = float(ratio[k])
            at = float("nan") if e32 is None else float(e32.detach().double().cpu().abs().reshape(-1)[k])
            self.rows[what] = (float(err.reshape(-1)[k]), at, float(allow.reshape(-1)[k]), where)
        ok = err <= allow                                  # (a NaN on either side fails)
        assert bool(ok.all()), (self.tag, what, where, "elements outside", int(ok.logical_not().sum()), "worst error / bound",
                                float(ratio[k]), "error", float(err.reshape(-1)[k]), "bound", float(allow.reshape(-1)[k]))

    def note(self, what, value, gate, where=""):
        """A scalar figure (units of a gate, a count) kept if it is the largest so far."""
        row = self.rows.get(what)
        if row is None or value > row[0]:
            self.rows[what] = (float(value), float("nan"), float(gate), where)

    def report(self):
        for what, (worst, e32, gate, where) in self.rows.items():
            print(f"{self.prefix} {self.tag:<44} {what:<12} kernel {worst:.3e}  torch-fp32 {e32:.3e}  gate {gate:.3e}"
                  f"{'  at ' + where if where else ''}")
