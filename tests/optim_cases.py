"""What the GPU tests of csrc/optim.hip share (tests/test_gpu_optim_kernels.py, tests/test_gpu_optim_recipe.py): every
tensor table lives inside ONE float32 allocation per role (param, grad, exp_avg, exp_avg_sq) with NaN guard words around
and between the tensors and a row without a gradient in the middle, so that a write outside a tensor is seen; the
gradients with the values that break a careless kernel; float32 rounding helpers."""
import torch

import optim

DEV = torch.device("cuda:0")
CHUNK = optim._CHUNK
ROLES = ("param", "grad", "exp_avg", "exp_avg_sq")
GUARD = 8                         # float32 words between and around the tensors
# a NaN: a guard word that is read as a gradient is also flagged by the overflow check, and poisons the norm
PATTERN = 0x7FC0BEEF
NULL_SIZE = 2049                  # the row without a gradient, in the middle of the table
SIZES = [1, 3, 4, 5, 1023, 1024, NULL_SIZE, 1025, 16383, 16384, 16385, 2 * 16384 + 7, 100003]
NULL_ROW = SIZES.index(NULL_SIZE)
# which roles start 4 bytes past a 16-byte boundary
SKEWS = {"aligned": (), "unaligned": ROLES, "grad_unaligned": ("grad",)}


def f32(x):
    """The float32 value of a Python float, as a Python float (what a C `float` argument receives)."""
    return float(torch.tensor(x, dtype=torch.float32))


def ulp(t):
    """Spacing of float32 at |t| (float64 tensor in, float64 out; 2^-149 at zero and among the denormals)."""
    a = t.abs().float()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


class Layout:
    """All tensors of one role inside one allocation: [guard] t0 [guard] t1 ... [guard]."""

    def __init__(self, skew=(), sizes=SIZES, null_row=NULL_ROW, seed=0):
        self.sizes, self.null_row = list(sizes), null_row
        self.live = [i for i in range(len(sizes)) if i != null_row]
        self.count = sum(self.sizes[i] for i in self.live)
        self.off = {}
        self.buf = {}
        g = torch.Generator().manual_seed(seed)
        for role in ROLES:
            offs, cur = [], GUARD
            for n in self.sizes:
                start = (cur + 3) // 4 * 4 + (1 if role in skew else 0)
                offs.append(start)
                cur = start + n + GUARD
            total = (cur + 3) // 4 * 4 + 4
            host = torch.full((total,), PATTERN, dtype=torch.int32).view(torch.float32)
            for i, (o, n) in enumerate(zip(offs, self.sizes)):
                if role == "param":
                    host[o:o + n] = torch.randn(n, generator=g)
                elif role == "exp_avg":
                    host[o:o + n] = 0.01 * torch.randn(n, generator=g)
                elif role == "exp_avg_sq":
                    host[o:o + n] = 1e-4 * torch.rand(n, generator=g)
                else:
                    host[o:o + n] = 0.1 * torch.randn(n, generator=g)
            self.off[role] = offs
            self.buf[role] = host.to(DEV)
            assert self.buf[role].data_ptr() % 16 == 0
        for role in ROLES:
            for i in range(len(self.sizes)):
                assert self.view(role, i).data_ptr() % 16 == (4 if role in skew else 0)
        self._keep = []

    def view(self, role, i):
        o = self.off[role][i]
        return self.buf[role][o:o + self.sizes[i]]

    def packed(self, role, rows=None):
        """The live tensors of one role, concatenated, on the host."""
        rows = self.live if rows is None else rows
        return torch.cat([self.view(role, i) for i in rows]).cpu()

    def set_packed(self, role, values):
        pos = 0
        for i in self.live:
            n = self.sizes[i]
            self.view(role, i).copy_(values[pos:pos + n])
            pos += n

    def position(self, i, j):
        """Index of element j of tensor i inside packed()."""
        return sum(self.sizes[k] for k in self.live if k < i) + j

    def bits(self):
        return {role: self.buf[role].view(torch.int32).cpu().clone() for role in ROLES}

    def restore(self, bits):
        for role in ROLES:
            self.buf[role].view(torch.int32).copy_(bits[role])

    def outside(self, role):
        """Mask of the words of `role` no kernel may write: the guards and the row without a gradient."""
        m = torch.ones(self.buf[role].numel(), dtype=torch.bool)
        for i in self.live:
            o = self.off[role][i]
            m[o:o + self.sizes[i]] = False
        return m

    def assert_outside_untouched(self, before, what):
        after = self.bits()
        for role in ROLES:
            m = self.outside(role)
            assert torch.equal(after[role][m], before[role][m]), "%s: wrote outside the tensors of %s" % (what, role)
        return after

    def table(self, first=True, second=True):
        """Device copies of the ru3d_adam_tensor table and the block map, as the fused optimizers build them (first /
        second: whether the rows name exp_avg / exp_avg_sq).  The row without a gradient keeps its state pointers: the
        kernel must leave it alone because its `grad` is null."""
        n = len(self.sizes)
        arr = (optim._AdamTensor * n)()
        blocks = []
        for i in range(n):
            arr[i] = optim._AdamTensor(self.view("param", i).data_ptr(),
                                       None if i == self.null_row else self.view("grad", i).data_ptr(),
                                       self.view("exp_avg", i).data_ptr() if first else None,
                                       self.view("exp_avg_sq", i).data_ptr() if second else None, self.sizes[i])
            for c in range((self.sizes[i] + CHUNK - 1) // CHUNK):
                blocks += [i, c]
        tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
        bm = torch.tensor(blocks, dtype=torch.int32).to(DEV)
        self._keep += [tab, bm]
        return tab, bm, len(blocks) // 2

    def optimizer(self, cls, **hp):
        """A fused optimizer over parameters, gradients and state that are views into the four allocations."""
        params = []
        for i in range(len(self.sizes)):
            p = torch.nn.Parameter(self.view("param", i))
            assert p.data_ptr() == self.view("param", i).data_ptr()
            params.append(p)
        opt = cls(params, **hp)
        for i in self.live:
            params[i].grad = self.view("grad", i)
            if cls is optim.SGD:
                if hp.get("momentum", 0) != 0:
                    opt.state[params[i]] = {"momentum_buffer": self.view("exp_avg", i)}
            else:
                opt.state[params[i]] = {"step": torch.tensor(0.0), "exp_avg": self.view("exp_avg", i),
                                        "exp_avg_sq": self.view("exp_avg_sq", i)}
        return opt, params

    def adam(self, **hp):
        """optim.Adam over parameters, gradients and moments that are views into the four allocations."""
        return self.optimizer(optim.Adam, **hp)


def make_grads(count, step, seed):
    """Normal gradients of both signs with exact zeros, 1e-30 (its square underflows) and 1e18 (its square is 1e36)."""
    g = torch.Generator().manual_seed(1000 * seed + step)
    v = 0.1 * torch.randn(count, generator=g)
    idx = torch.arange(count)
    sign = torch.where(v < 0, -1.0, 1.0)
    v[idx % 7 == 0] = 0.0
    v[idx % 11 == 0] = (1e-30 * sign)[idx % 11 == 0]
    v[idx % 13 == 0] = (1e18 * sign)[idx % 13 == 0]
    return v
