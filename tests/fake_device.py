"""A CPU tensor that says it is on a GPU: what lets the CPU tests reach the argument checks that come after a wrapper's device
check (dtype, requires_grad, device mismatch).  Only for calls that are refused: nothing may launch on it."""
import torch


class OnGpu(torch.Tensor):
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda", 1))

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t, t.requires_grad)
