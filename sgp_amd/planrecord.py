"""What the four host-built hop plans (``tileplan.TilePlan``, ``mixplan.MixPlan``, ``splitplan.SplitPlan``,
``colblock.ColBlockPlan``) share: a plan is a record of declared fields -- tensors, numbers, strings and dicts / lists /
tuples of them -- and ``PlanRecord`` moves such a record to a device (``to``) and turns it into the plain structure the
plan cache stores (``state`` / ``from_state``, sgp_amd/plancache.py).  A class declares its fields ONCE: as a dataclass,
or in a class-level ``FIELDS`` tuple; a field the class does not declare does not exist for any of the three."""
import dataclasses

import numpy as np
import torch


def _walk(v, leaf):
    """``v`` with ``leaf`` applied to everything that is not a dict, list or tuple (dict keys included); containers are
    rebuilt."""
    if isinstance(v, dict):
        return {leaf(k): _walk(x, leaf) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_walk(x, leaf) for x in v)
    return leaf(v)


def _plain(v):
    """A leaf as ``torch.load(weights_only=True)`` takes it back: numpy scalars and arrays become Python numbers and tensors."""
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(v))
    if v is None or torch.is_tensor(v) or isinstance(v, (bool, int, float, str)):
        return v
    raise TypeError(f"a plan field holds a {type(v).__name__}: neither a tensor, a number, a string nor a container of them")


class PlanRecord:
    KIND = None          # tag of the class in a stored state (plancache's kind -> class table)
    FIELDS = ()          # the declared fields of a class that is no dataclass
    HOST = ()            # fields that stay where they are: carried by reference through ``to``, left out of ``state``

    @classmethod
    def field_names(cls):
        return tuple(f.name for f in dataclasses.fields(cls)) if dataclasses.is_dataclass(cls) else cls.FIELDS

    @classmethod
    def _of(cls, values):
        new = object.__new__(cls)
        new.__dict__.update(values)
        return new

    def to(self, device):
        """A new plan of the same class with every tensor, at any depth, on ``device``; the rest is carried over."""
        move = lambda v: v.to(device) if torch.is_tensor(v) else v
        return self._of({k: getattr(self, k) if k in self.HOST else _walk(getattr(self, k), move)
                         for k in self.field_names()})

    def state(self):
        """The plan as dicts, lists, tuples, tensors, numbers, strings and None, tagged with its ``kind``."""
        st = {k: _walk(getattr(self, k), _plain) for k in self.field_names() if k not in self.HOST}
        st["kind"] = self.KIND
        return st

    @classmethod
    def from_state(cls, state):
        """Inverse of ``state``; a state of another kind or without one of the declared fields raises."""
        if state["kind"] != cls.KIND:
            raise ValueError(f"a {state['kind']!r} state is no {cls.KIND!r} plan")
        return cls._of({k: _walk(state[k], lambda v: v) for k in cls.field_names() if k not in cls.HOST})
