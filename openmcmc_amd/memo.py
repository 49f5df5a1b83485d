"""Memo keyed by object identity: for what is derived once from shared, immutable host objects (a precision matrix, a design
matrix, a response) and reused every sweep."""

from operator import is_


def by_identity(memo, make, *objs):
    """The value `make()` gave for these very objects, made and stored in the dict `memo` on first request.

    An id can be recycled once its object is collected, so the entry keeps the objects it was made from and counts as a hit
    only if every one of them IS the object asked about; anything else calls `make` again and replaces the entry."""
    key = tuple(map(id, objs))
    hit = memo.get(key)
    if hit is not None and len(hit[0]) == len(objs) and all(map(is_, hit[0], objs)):
        return hit[1]
    value = make()
    memo[key] = (objs, value)
    return value
