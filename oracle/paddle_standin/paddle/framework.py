"""paddle.framework of the stand-in: ParamAttr (table entry L8)."""


class ParamAttr:
    def __init__(self, name=None, initializer=None, trainable=True):
        self.name, self.initializer, self.trainable = name, initializer, trainable


def __getattr__(name):
    raise AttributeError("paddle.framework stand-in: '%s' is not one of the names the reference's model code uses" % name)
