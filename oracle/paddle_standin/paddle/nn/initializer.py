"""paddle.nn.initializer of the stand-in: Assign (table entry L8)."""


class Assign:
    def __init__(self, value):
        self.value = value


def __getattr__(name):
    raise AttributeError("paddle.nn.initializer stand-in: '%s' is not one of the names the reference's model code uses" % name)
